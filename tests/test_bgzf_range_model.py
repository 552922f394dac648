"""The range rule and the argument checks of flate_hip_bgzf_read_ranges on the CPU:
moonbit-flate_amd/csrc/bgzf_range_rule.h -- the one function the locate kernel and the library's host code compile --
and api_checks.h's bgzf_ranges_args, built with g++ into a stand-alone program under AddressSanitizer and UBSan, run
over every well-formed file of the corpus (index and range arrays in allocations of exactly their size) with range
lists that sit on every edge, and compared with the Python model tests/bgzf_range_ref.py.  The same program runs
range_statuses, the status rule behind the decode of every ranges call, over hand-made cases."""
import os
import struct
import subprocess

import pytest

import bgzf_range_ref as model
import bgzf_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "bgzf_range_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(CSRC, "bgzf_range_rule.h"), os.path.join(CSRC, "bgzf_rule.h"),
        os.path.join(CSRC, "api_checks.h"), os.path.join(INC, "flate_hip.h")]
EXE = os.path.join(HERE, "host_model", "bgzf_range_model")
INVALID = -1


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + INC, SRC, "-o", EXE])
    return EXE


@pytest.fixture(scope="module")
def cases():
    """[(what, file, kind, ranges)] over every well-formed file of the corpus."""
    out = []
    for what, f in ref.index_corpus():
        w = ref.Walk(f)
        if w.rc:
            continue
        out.append((what, f, model.POS_BYTES, model.byte_edge_ranges(w)))
        out.append((what, f, model.POS_VIRTUAL, model.virtual_edge_ranges(f, w)))
    return out


def test_the_range_lists_reach_every_kind_of_end_point(cases):
    seen = set()
    for what, f, kind, ranges in cases:
        w = ref.Walk(f)
        if kind != model.POS_VIRTUAL:
            assert (w.out_bytes + 1, model.U64_MAX) in ranges and (0, w.out_bytes) in ranges, what
            continue
        decoys = set(model.decoy_offsets(f, w))
        for b, e in ranges:
            for v in (b, e):
                c, u = v >> 16, v & 0xffff
                if c in decoys:
                    seen.add("decoy")
                elif c == len(f):
                    seen.add("end+%d" % u)
                elif c in w.member_off:
                    k = w.member_off.index(c)
                    seen.add("isize%+d" % (u - (w.out_off[k + 1] - w.out_off[k])) if u > 1 else "u%d" % u)
                elif c < len(f):
                    seen.add("inside")
    assert {"decoy", "end+0", "end+1", "inside", "u0", "u1", "isize-1", "isize+0", "isize+1"} <= seen, seen


def test_rule_equals_the_python_model_on_every_file(exe, cases, tmp_path):
    blob = struct.pack("<I", len(cases))
    for _, f, kind, ranges in cases:
        blob += struct.pack("<Q", len(f)) + f + struct.pack("<II", kind, len(ranges))
        blob += struct.pack("<%dQ" % len(ranges), *[b for b, _ in ranges]) + struct.pack("<%dQ" % len(ranges), *[e for _, e in ranges])
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    lines = subprocess.run([exe, "locate", str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(cases)
    n_invalid = n_valid = 0
    for (what, f, kind, ranges), line in zip(cases, lines):
        w = ref.Walk(f)
        got = [[int(x) for x in part.split()] for part in line.split(";") if part]
        assert len(got) == len(ranges), what
        for (b, e), g in zip(ranges, got):
            x = model.locate(kind, b, e, w)
            if x is None:
                assert g == [INVALID, 0, 0, -1, -1], (what, kind, b, e, g)
                n_invalid += 1
                continue
            ks = model.members_of(w, x[0], x[1])
            assert g == [0, x[0], x[1], ks[0] if ks else -1, ks[-1] if ks else -1], (what, kind, b, e, g)
            n_valid += 1
    assert n_invalid > 100 and n_valid > 1000


def test_argument_checks(exe):
    out = subprocess.run([exe, "checks"], check=True, capture_output=True, text=True).stdout
    got = dict((k, int(v)) for k, v in (line.split() for line in out.splitlines()))
    assert got == {
        "ok_bytes": 0, "ok_virtual_device": 0, "ok_size_query": 0, "ok_empty_file": 0, "ok_no_ranges": 0,
        "ok_equal_ends": 0,
        "no_in": INVALID, "no_begin": INVALID, "no_end": INVALID, "no_out_off": INVALID, "no_out_with_cap": INVALID,
        "kind_2": INVALID, "kind_max": INVALID, "flag_go": INVALID, "flag_size_only": INVALID,
        "backwards_bytes": INVALID, "backwards_virtual": INVALID, "backwards_not_reached": 0,
    }


CORRUPT, EOF_ = -3, -4  # (any two distinct non-zero statuses: the rule copies them)

# (what, st, [(r_lo, r_hi)], the statuses the ranges start with, skip or None)
STATUS_CASES = [
    ("no bad unit", [0, 0, 0, 0, 0, 0, 0], [(0, 2), (2, 5), (5, 7)], [0, 0, 0], None),
    ("bad in the first range", [0, CORRUPT, 0, 0, 0, 0, 0], [(0, 2), (2, 5), (5, 7)], [0, 0, 0], None),
    ("bad in a middle range", [0, 0, 0, CORRUPT, 0, 0, 0], [(0, 2), (2, 5), (5, 7)], [0, 0, 0], None),
    ("bad in the last range, its last unit", [0, 0, 0, 0, 0, 0, EOF_], [(0, 2), (2, 5), (5, 7)], [0, 0, 0], None),
    ("two ranges share the bad unit", [0, 0, CORRUPT, 0, 0], [(0, 3), (2, 5), (3, 5)], [0, 0, 0], None),
    ("the first of two bad units in a range wins", [0, EOF_, CORRUPT, 0], [(0, 4), (2, 4)], [0, 0], None),
    ("an empty range keeps its status", [CORRUPT, 0, 0], [(0, 0), (1, 1), (3, 3), (0, 3)], [0, 7, 0, 0], None),
    ("a range outside the decoded units keeps its status", [CORRUPT, 0], [(0, 3), (0, 2)], [5, 0], None),
    ("a range settled before the decode keeps its status", [CORRUPT, 0, 0], [(0, 2), (0, 2), (1, 3)], [-1, 0, 0], [-1, 0, 0]),
    ("skip given, nothing skipped", [0, 0, EOF_], [(0, 3), (2, 3)], [0, 0], [0, 0]),
    ("no status array", [0, CORRUPT, 0], [(0, 3)], [9], None),
    ("no units, no ranges", [], [], [], None),
    ("unsorted, nested and repeated ranges", [0, 0, CORRUPT, 0, EOF_, 0], [(4, 6), (0, 6), (3, 4), (0, 6), (1, 3)], [0, 0, 0, 0, 0], None),
]


def _statuses_model(st, ranges, start, skip):
    """The rule, the slow way: every range looks at every unit it touches."""
    out = list(start)
    for r, (lo, hi) in enumerate(ranges):
        if (skip and skip[r]) or hi > len(st):
            continue
        bad = [st[i] for i in range(lo, hi) if st[i]]
        if bad:
            out[r] = bad[0]
    first = [i for i, s in enumerate(st) if s]
    return (first[0] if first else len(st)), out


def test_status_rule_behind_the_decode(exe, tmp_path):
    text = ""
    for what, st, ranges, start, skip in STATUS_CASES:
        with_status = 0 if what == "no status array" else 1
        nums = [len(st), len(ranges), 1 if skip is not None else 0, with_status] + st + [a for a, _ in ranges] + \
               [b for _, b in ranges] + start + (skip if skip is not None else [0] * len(ranges))
        text += " ".join(str(x) for x in nums) + "\n"
    path = tmp_path / "statuses.txt"
    path.write_text(text)
    lines = subprocess.run([exe, "statuses", str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(STATUS_CASES)
    for (what, st, ranges, start, skip), line in zip(STATUS_CASES, lines):
        got = [int(x) for x in line.split()]
        first, want = _statuses_model(st, ranges, start, skip)
        if what == "no status array":
            want = list(start)
        assert got[0] == first, what
        assert got[1:] == want, what
    # what the cases are for, spelled out
    by = dict((c[0], _statuses_model(*c[1:])) for c in STATUS_CASES)
    assert by["no bad unit"] == (7, [0, 0, 0])
    assert by["bad in a middle range"] == (3, [0, CORRUPT, 0])
    assert by["two ranges share the bad unit"] == (2, [CORRUPT, CORRUPT, 0])
    assert by["a range settled before the decode keeps its status"] == (0, [-1, CORRUPT, 0])
