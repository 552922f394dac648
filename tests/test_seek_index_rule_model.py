"""The seek index's rule and the argument checks of its two calls on the CPU: moonbit-flate_amd/csrc/seek_index_rule.h
-- the functions the kernels and the library's host code compile -- and api_checks.h's one_seek_index_args /
one_ranges_args, built with g++ into a stand-alone program under AddressSanitizer and UBSan, run over the corpus of
tests/one_ref.py (arrays in allocations of exactly their size) and compared with the Python model tests/seek_ref.py."""
import os
import struct
import subprocess

import pytest

import one_ref as ref
import seek_ref as sk

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "seek_index_rule_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(CSRC, "seek_index_rule.h"), os.path.join(CSRC, "bgzf_range_rule.h"), os.path.join(CSRC, "bgzf_rule.h"),
        os.path.join(CSRC, "api_checks.h"), os.path.join(INC, "flate_hip.h")]
EXE = os.path.join(HERE, "host_model", "seek_index_rule_model")
SPANS = (1, 4096, 40000, 100000, 0, sk.SPAN_NONE)
INVALID = -1


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + INC, SRC, "-o", EXE])
    return EXE


@pytest.fixture(scope="module")
def walks():
    """[(what, raw stream, plain, Walk)]: computed once, shared, never changed."""
    return [(what, raw, plain, ref.Walk(raw)) for what, raw, plain in ref.good_streams()]


def test_the_spans_cut_the_many_unit_stream_as_the_gpu_tests_need(walks):
    w = walks[ref.MANY_UNITS][3]
    assert len(sk.points(w.out_off, 1)) == w.n_units
    assert len(sk.points(w.out_off, 4096)) >= 50
    pts = sk.points(w.out_off, 100000)
    assert max(b - a for a, b in zip(pts, pts[1:] + [w.n_units])) >= 64
    assert sk.points(w.out_off, sk.SPAN_NONE) == [0] == sk.points(w.out_off, 0)  # (300 000 bytes: inside the first MiB)


def test_points_locate_and_decoded_sets_equal_the_python_model(exe, walks, tmp_path):
    cases = []
    for what, raw, plain, w in walks:
        for span in SPANS:
            pts = sk.points(w.out_off, span)
            cases.append((what, w, span, pts, sk.edge_ranges(w.out_off, pts)))
        k = sk.longest_segment_last(w.out_off, sk.points(w.out_off, 100000))
        if w.out_off[k + 1] > w.out_off[k]:  # one byte in the last unit of the longest segment, alone
            cases.append((what, w, 100000, sk.points(w.out_off, 100000), [(w.out_off[k + 1] - 1, w.out_off[k + 1])]))
    blob = struct.pack("<I", len(cases))
    for _, w, span, _, ranges in cases:
        blob += struct.pack("<QI", span, w.n_units) + struct.pack("<%dQ" % (w.n_units + 1), *w.out_off)
        blob += struct.pack("<I", len(ranges)) + struct.pack("<%dQ" % len(ranges), *[b for b, _ in ranges])
        blob += struct.pack("<%dQ" % len(ranges), *[e for _, e in ranges])
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    lines = subprocess.run([exe, "rule", str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(cases)
    n_ranges = n_partial = 0
    for (what, w, span, pts, ranges), line in zip(cases, lines):
        got_pts, got_loc, got_dec = line.split("|")
        assert [int(x) for x in got_pts.split()] == pts, (what, span)
        locs = [[int(x) for x in part.split()] for part in got_loc.split(";") if part]
        assert len(locs) == len(ranges), (what, span)
        for (begin, end), g in zip(ranges, locs):
            b, e, first, last = sk.locate(w.out_off, begin, end)
            want = [b, e, -1, -1, -1] if first is None else [b, e, first, last, sk.pstart(pts, first)]
            assert g == want, (what, span, begin, end, g)
            n_ranges += 1
        dec = sorted(sk.decoded(w.out_off, pts, ranges))
        assert [int(x) for x in got_dec.split()] == dec, (what, span)
        if len(ranges) == 1 and w is walks[ref.MANY_UNITS][3]:  # the one byte: its segment up to its unit, no more
            k = sk.longest_segment_last(w.out_off, pts)
            assert dec == list(range(sk.pstart(pts, k), k + 1)) and 64 <= len(dec) < w.n_units
            n_partial += 1
    assert n_ranges > 5000 and n_partial == 1


def test_seek_index_ok_refuses_one_violation_of_every_clause(exe, walks, tmp_path):
    what, raw, plain, w = walks[ref.MANY_UNITS]
    cases = []
    for kind in (ref.RAW, ref.ZLIB, ref.GZIP):
        for span in SPANS:
            words = sk.index_words(w, plain, len(raw), kind, span)
            in_len = len(ref.wrap(raw, plain, kind))
            cases.append(("sound", words, (words[9] - 1) * sk.WINDOW, kind, in_len, True))
    words = sk.index_words(w, plain, len(raw), ref.GZIP, 4096)
    in_len = len(ref.wrap(raw, plain, ref.GZIP))
    bent = list(words)
    bent[sk.HEAD_WORDS + 100] += 1  # moved by one bit: still strictly increasing, still sound
    cases.append(("an interior unit_bit moved by one bit", bent, (words[9] - 1) * sk.WINDOW, ref.GZIP, in_len, True))
    for v in sk.violations(words, (words[9] - 1) * sk.WINDOW, ref.GZIP, in_len):
        cases.append(v + (False,))
    for k in (7, 11):  # a stream of one unit and the empty stream
        _, r2, p2, w2 = walks[k]
        wd = sk.index_words(w2, p2, len(r2), ref.ZLIB, 1)
        cases.append((walks[k][0], wd, 0, ref.ZLIB, len(ref.wrap(r2, p2, ref.ZLIB)), True))
    cases.append(("fewer words than the head", words[:sk.HEAD_WORDS - 1], 0, ref.GZIP, in_len, False))
    cases.append(("no words", [], 0, ref.GZIP, in_len, False))
    blob = struct.pack("<I", len(cases))
    for _, wd, wb, kind, n, _ in cases:
        blob += struct.pack("<IQQQ", kind, n, wb & sk.U64, len(wd)) + struct.pack("<%dQ" % len(wd), *[x & sk.U64 for x in wd])
    path = tmp_path / "index.bin"
    path.write_bytes(blob)
    lines = subprocess.run([exe, "ok", str(path)], check=True, capture_output=True, text=True).stdout.split()
    assert len(lines) == len(cases)
    for (what, wd, wb, kind, n, want), got in zip(cases, lines):
        assert sk.index_ok(wd, wb, kind, n) == want, what  # the Python model agrees with the hand-made verdict ...
        assert (got == "1") == want, what                   # ... and so does the header


def test_argument_checks(exe):
    out = subprocess.run([exe, "checks"], check=True, capture_output=True, text=True).stdout
    got = dict((k, int(v)) for k, v in (line.split() for line in out.splitlines()))
    assert got == {
        "build_ok": 0, "build_query": 0, "build_empty_input": 0,
        "build_no_in": INVALID, "build_no_index_with_cap": INVALID, "build_no_windows_with_cap": INVALID,
        "build_no_index_words": INVALID, "build_no_windows_bytes": INVALID, "build_no_n_units": INVALID,
        "build_no_n_points": INVALID, "build_no_out_bytes": INVALID, "build_no_status": INVALID, "build_wrap_3": INVALID,
        "build_flag_go": INVALID,
        "read_ok": 0, "read_size_query": 0, "read_no_ranges": 0,
        "read_no_index": INVALID, "read_no_begin": INVALID, "read_no_out_off": INVALID, "read_no_out_with_cap": INVALID,
        "read_backwards": INVALID, "read_wrap_3": INVALID, "read_wrap_not_the_index": INVALID,
        "read_windows_without_buffer": INVALID, "read_flag_size_only": INVALID,
    }
