"""The rule of a gzip file's seek index and the argument checks of its two calls on the CPU:
moonbit-flate_amd/csrc/gzfile_seek_rule.h -- the functions the kernels and the library's host code compile -- and
api_checks.h's gzfile_seek_index_args / gzfile_ranges_args, built with g++ into a stand-alone program under
AddressSanitizer and UBSan, run over the corpus of tests/gzfile_seek_ref.py and tests/gzfile_ref.py (arrays in
allocations of exactly their size) and compared with the Python model tests/gzfile_seek_ref.py."""
import os
import struct
import subprocess

import pytest

import gzfile_ref as gzf
import gzfile_seek_ref as R
import seek_ref as sk

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "gzfile_seek_rule_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(INC, "flate_hip.h")] + [os.path.join(CSRC, h) for h in (
    "gzfile_seek_rule.h", "seek_index_rule.h", "bgzf_range_rule.h", "bgzf_rule.h", "api_checks.h")]
EXE = os.path.join(HERE, "host_model", "gzfile_seek_rule_model")
INVALID = -1
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + INC, SRC, "-o", EXE])
    return EXE


@pytest.fixture(scope="module")
def files():
    """[(what, file, plain, Walk)]: computed once, shared, never changed."""
    out = [("seek_file",) + R.seek_file(), ("tiny_file",) + gzf.tiny_file()]
    pm = gzf.phase_members()
    out.append(("phase_members", b"".join(m for m, _ in pm), b"".join(p for _, p in pm)))
    out.append(("history_files",) + gzf.history_files()[:2])
    tm = gzf.three_members()
    out.append(("three_members", b"".join(m for m, _ in tm), b"".join(p for _, p in tm)))
    out += gzf.tile_edge_files()[:4]
    return [(what, f, plain, gzf.Walk(f)) for what, f, plain in out]


def test_the_corpus_reaches_every_edge(files):
    what, f, plain, w = files[0]
    assert b"".join(gzf.members_of(f)) == plain and w.status == 0
    assert (w.n_members, w.out_off[-1]) == (6, len(plain)) and w.n_units >= 200
    assert any(w.out_off[k + 1] == w.out_off[k] for k in range(w.n_units))  # the empty member's unit
    for span in R.SPANS:
        pts = R.points(w, span)
        assert set(R.starts(w)) <= set(pts)
        assert all(R.first_unit(w, a) == R.first_unit(w, a + c - 1) for a, c in R.segments(w.n_units, pts))  # no segment crosses a member
    assert R.windows_bytes(w, 1) > 0 and R.windows_bytes(w, 4096) > 0 and R.windows_bytes(w, 100000) > 0
    assert len(R.partial(w, R.points(w, 4096))) > 0
    assert any(R.first_unit(w, u) != 0 for u in R.partial(w, R.points(w, 4096)))  # ... with another member in front
    assert max(c for _, c in R.segments(w.n_units, R.points(w, 100000))) >= 64  # a seven-step segmented scan
    assert set(R.starts(w)) - set(sk.points(w.out_off, 4096))  # a member start that the span rule alone does not make
    assert R.points(w, R.SPAN_NONE) == R.starts(w) and R.windows_bytes(w, R.SPAN_NONE) == 0
    # a window of a partial point: zeros where U has the bytes of the member in front
    pts = R.points(w, 4096)
    u = next(u for u in R.partial(w, pts) if R.first_unit(w, u) != 0)
    blk, zeros = R.window(w, plain, u), R.WINDOW - R.rel(w, u)
    assert blk[:zeros] == b"\0" * zeros and sk.window(plain, w.out_off[u])[:zeros].strip(b"\0")
    assert R.windows(w, plain, pts)[R.block(w, pts, pts.index(u)) * R.WINDOW:][:R.WINDOW] == blk


def test_points_blocks_locate_and_decoded_sets_equal_the_python_model(exe, files, tmp_path):
    cases = []
    for what, f, plain, w in files:
        for span in R.SPANS:
            pts = R.points(w, span)
            cases.append((what, w, span, pts, R.edge_ranges(w, pts)))
    blob = struct.pack("<I", len(cases))
    for _, w, span, _, ranges in cases:
        blob += struct.pack("<QI", span, w.n_units) + struct.pack("<%dQ" % (w.n_units + 1), *w.out_off)
        blob += struct.pack("<I", w.n_members) + struct.pack("<%dQ" % (w.n_members + 1), *w.member_unit)
        blob += struct.pack("<I", len(ranges)) + struct.pack("<%dQ" % len(ranges), *[b for b, _ in ranges])
        blob += struct.pack("<%dQ" % len(ranges), *[e for _, e in ranges])
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    lines = subprocess.run([exe, "rule", str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(cases)
    n_ranges = n_windows = 0
    for (what, w, span, pts, ranges), line in zip(cases, lines):
        got_pts, got_loc, got_dec, got_units = line.split("|")
        want_pts, before = [], 0
        for p, u in enumerate(pts):
            b = R.block(w, pts, p)
            want_pts.append("%d:%d[%d]" % (u, -1 if b is None else b, before))
            assert b is None or b == before, (what, span, u)  # the blocks are numbered in stream order without a gap
            before += b is not None
        assert got_pts.split() == want_pts, (what, span)
        n_windows += before
        locs = [[int(x) for x in part.split()] for part in got_loc.split(";") if part]
        assert len(locs) == len(ranges), (what, span)
        for (begin, end), g in zip(ranges, locs):
            b, e, first, last = sk.locate(w.out_off, begin, end)
            want = [b, e, -1, -1, -1] if first is None else [b, e, first, last, sk.pstart(pts, first)]
            assert g == want, (what, span, begin, end, g)
            n_ranges += 1
        assert [int(x) for x in got_dec.split()] == sorted(R.decoded(w, pts, ranges)), (what, span)
        units = [[int(x) for x in part.split()] for part in got_units.split(";") if part]
        nxt = set(w.member_unit)
        assert units == [[R.rel(w, k), min(R.WINDOW, R.rel(w, k)), int(k + 1 in nxt)] for k in range(w.n_units)], (what, span)
    assert n_ranges > 5000 and n_windows > 300


def test_index_ok_refuses_one_violation_of_every_clause(exe, files, tmp_path):
    what, f, plain, w = files[0]
    cases = []
    for what2, f2, _, w2 in files:
        for span in R.SPANS:
            cases.append(("sound: " + what2, R.index_words(w2, len(f2), span), R.windows_bytes(w2, span), len(f2), True))
    words, wb = R.index_words(w, len(f), 4096), R.windows_bytes(w, 4096)
    bent = list(words)
    bent[R.HEAD_WORDS + 100] += 1  # moved by one bit: still strictly increasing, still sound
    cases.append(("an interior unit_bit moved by one bit", bent, wb, len(f), True))
    for v in R.violations(words, wb, len(f)):
        cases.append(v + (False,))
    empty = R.index_words(gzf.Walk(b""), 0, 0)
    cases.append(("the empty file", empty, 0, 0, True))
    cases.append(("the empty file's head for a file of bytes", empty[:2] + [5] + empty[3:], 0, 5, False))
    cases.append(("the empty file's head with windows", empty, R.WINDOW, 0, False))
    cases.append(("the empty file's head with a total", empty[:3] + [1] + empty[4:], 0, 0, False))
    cases.append(("the empty file's head and a word", empty + [0], 0, 0, False))
    cases.append(("fewer words than the head", words[:R.HEAD_WORDS - 1], 0, len(f), False))
    cases.append(("no words", [], 0, len(f), False))
    blob = struct.pack("<I", len(cases))
    for _, wd, b, n, _ in cases:
        blob += struct.pack("<QQQ", n, b & U64, len(wd)) + struct.pack("<%dQ" % len(wd), *[x & U64 for x in wd])
    path = tmp_path / "index.bin"
    path.write_bytes(blob)
    lines = subprocess.run([exe, "ok", str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(cases)
    for (what, wd, b, n, want), line in zip(cases, lines):
        got, size_w, size_b = (int(x) for x in line.split())
        assert R.index_ok(wd, b, n) == want, what  # the Python model agrees with the hand-made verdict ...
        assert (got == 1) == want, what              # ... and so does the header
        if want:
            assert (size_w, size_b) == (len(wd), b), what  # gzfile_seek_index_words / gzfile_seek_windows_bytes


def test_argument_checks(exe):
    out = subprocess.run([exe, "checks"], check=True, capture_output=True, text=True).stdout
    got = dict((k, int(v)) for k, v in (line.split() for line in out.splitlines()))
    assert got == {
        "build_ok": 0, "build_query": 0, "build_empty_input": 0,
        "build_no_in": INVALID, "build_no_index_with_cap": INVALID, "build_no_windows_with_cap": INVALID,
        "build_no_index_words": INVALID, "build_no_windows_bytes": INVALID, "build_no_n_units": INVALID,
        "build_no_n_members": INVALID, "build_no_n_points": INVALID, "build_no_out_bytes": INVALID,
        "build_no_status": INVALID, "build_flag_go": INVALID,
        "read_ok": 0, "read_size_query": 0, "read_no_ranges": 0, "read_empty_file": 0,
        "read_no_in": INVALID, "read_no_index": INVALID, "read_no_begin": INVALID, "read_no_end": INVALID,
        "read_no_out_off": INVALID, "read_no_out_with_cap": INVALID, "read_backwards": INVALID,
        "read_in_len_not_the_index": INVALID, "read_windows_without_buffer": INVALID,
        "read_windows_the_index_has_not": INVALID, "read_flag_size_only": INVALID,
    }
