"""The rule of a gzip FILE read in parts with short members decoded WHOLE, on the CPU:
moonbit-flate_amd/csrc/gzfile_parts_serial_rule.h -- the functions the kernels and flate_hip_gzfile_reader_read compile
-- and api_checks.h's gzfile_reader_set_serial_max_args / _last_route_args, built with g++ into a stand-alone program
under AddressSanitizer and UBSan and compared with the Python reference tests/gzfile_parts_serial_ref.py: THE THREE
VERDICTS at every cut of a trailer plus a header with FNAME, final and not; whole readers -- every call's eight words
and its route -- at every cut of two small files for S in (64, 4096) and out_cap in (None, 300), a call that is
FLATE_HIP_E_OUT_TOO_SMALL repeated with the capacity it asked for; and gzfile_serial_ref.mixed_file() at cuts every
997 bytes with S = 4096."""
import os
import subprocess

import pytest

import gzfile_parts_serial_ref as R
import gzfile_ref as gf
import gzfile_serial_ref as gs
import gzip_ref as gz
from test_gzfile_parts_rule_model import hexs, world

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "gzfile_parts_serial_rule_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(INC, "flate_hip.h")] + [os.path.join(CSRC, h) for h in (
    "gzfile_parts_serial_rule.h", "gzfile_parts_rule.h", "gzfile_serial_rule.h", "gzfile_rule.h", "one_parts_rule.h",
    "api_checks.h", "gzip_rule.h")]
EXE = os.path.join(HERE, "host_model", "gzfile_parts_serial_rule_model")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + INC, SRC, "-o", EXE])
    return EXE


def run(exe, lines, tmp_path):
    p = tmp_path / "commands.txt"
    p.write_text("\n".join(lines) + "\n")
    return subprocess.check_output([exe, "run", str(p)]).decode().split("\n")[:-1]


# ---- the three verdicts ----

def test_the_verdicts_at_every_cut_of_a_trailer_and_a_header(exe, tmp_path):
    t = gz.text(900, seed=3)
    first = gz.member(t[:200], 6)
    second = gz.member(t[200:], 6, flg=gz.FNAME, name=b"a name")
    f = first + second + gz.fixed(b"end")
    lines, want = [], []
    for cut in range(len(first) - 8, len(f) + 1):
        part = f[:cut]
        for p in gs.table(part):
            for final in (0, 1):
                for S, out_cap in ((4096, 1 << 62), (64, 1 << 62), (len(second), 1 << 62), (4096, 300)):
                    hl, E, st, used, size = gs.candidate(part, p, S)
                    lines.append("V %d %d %d %d %d %d %d %s" % (final, S, out_cap, p, st, used, size, hexs(part)))
                    want.append("%d" % R.verdict(part, p, S, bool(final), out_cap)[0])
    got = run(exe, lines, tmp_path)
    assert got == want, [(i, lines[i][:40], g, x) for i, (g, x) in enumerate(zip(got, want)) if g != x][:3]
    assert {x for x in want} == {"0", "1", "2"}  # every answer occurs


# ---- whole readers ----

class Recorded:
    def __init__(self, m):
        self.m, self.lines, self.expect = m, world(m), []
        self.cands = {}  # (the candidate's file offset, the part's end) -> "used z s"

    def fresh(self):
        self.m.reset()
        self.lines.append("N %d %d" % (self.m.unit_max, self.m.S))
        self.model_read = R.model_reader(self.m)

    def read(self, buf, final, out_cap):
        a, m = self.m.consumed, self.m
        words = []
        if m.S:
            for p in gs.table(buf):
                key = (a + p, a + len(buf))
                if key not in self.cands:
                    _, _, st, used, size = gs.candidate(buf, p, m.S)
                    self.cands[key] = "%d %d %d" % (used, size, st)
                words.append("%d %s" % (p, self.cands[key]))
        self.lines.append("C %d %s" % (len(words), " ".join(words)))
        self.lines.append("R %d %d %d" % (len(buf), final, out_cap if out_cap is not None else 1 << 62))
        c, got = self.model_read(buf, final, out_cap)
        self.expect.append(tuple(c) + self.m.route)
        return c, got

    def check(self, exe, tmp_path, what):
        got = run(exe, self.lines, tmp_path)
        want = [" ".join("%d" % x for x in c) for c in self.expect]
        assert got == want, (what, [(i, g, x) for i, (g, x) in enumerate(zip(got, want)) if g != x][:3])


def files():
    three = b"".join(x for x, _ in gf.three_members())
    return [("three_members", three), ("tiny_file", gf.tiny_file()[0])]


def growing(read):
    """`read` of feed() that repeats a call that was FLATE_HIP_E_OUT_TOO_SMALL with the capacity it asked for."""
    def again(buf, final, out_cap):
        c, got = read(buf, final, out_cap)
        if c.rc == R.OUT_TOO_SMALL:
            c, got = read(buf, final, c.out_len)
        return c, got
    return again


@pytest.mark.parametrize("S", (64, 4096))
@pytest.mark.parametrize("what,f", files(), ids=[x for x, _ in files()])
def test_whole_readers_at_every_cut(exe, tmp_path, what, f, S):
    plain = b"".join(gf.members_of(f))
    rec = Recorded(R.Model(f, S))
    for cut in range(0, len(f) + 1):
        rec.fresh()
        calls, out, rest = R.feed(rec.read, f, [cut], None, 8, grow=len(f))
        assert calls[-1].rc == R.STREAM_END and out == plain and not rest, cut
    for cut in range(0, len(f) + 1):
        rec.fresh()
        calls, out, rest = R.feed(growing(rec.read), f, [cut], 300, 4000, grow=len(f))
        assert calls[-1].rc == R.STREAM_END and out == plain and not rest, cut
    rec.check(exe, tmp_path, (what, S))


def test_long_and_short_members_at_cuts_every_997_bytes(exe, tmp_path):
    f, plain, long_ones = gs.mixed_file()
    rec = Recorded(R.Model(f, 4096))
    for cut in range(0, len(f) + 1, 997):
        rec.fresh()
        calls, out, rest = R.feed(rec.read, f, [cut], None, 8, grow=len(f))
        assert calls[-1].rc == R.STREAM_END and out == plain and not rest, cut
    rec.fresh()
    calls, out, rest = R.feed(rec.read, f, iter(lambda: 997, 0), None, 4000, grow=997)
    assert calls[-1].rc == R.STREAM_END and out == plain
    rec.check(exe, tmp_path, "mixed_file")


# ---- the whole file is the part that is final and starts at a BOUNDARY: what the one set of kernels rests on ----

@pytest.fixture(scope="module")
def equalities(exe):
    lines = subprocess.check_output([exe, "equalities"]).decode().split("\n")[:-1]
    return {t[0]: t[1:] for t in (line.split() for line in lines)}


def test_the_parts_hop_of_a_final_part_is_the_hop(equalities):
    """Every end bit of seven buffers of at most 64 bytes: a trailer, then the end, a good header, a bad byte, a header
    cut in three ways or a reserved FLG bit; kind, e and bit agree, and every kind and e > in_len occur."""
    t = equalities["hop"]
    assert int(t[0]) > 1000 and int(t[1]) == 0, t
    assert t[2::2] == ["end", "dead", "next", "beyond"] and all(int(x) > 0 for x in t[3::2]), t


def test_the_verdict_of_a_final_part_without_a_cap_is_the_whole_test(equalities):
    """in_len <= 48, every p and used, four header lengths, five statuses, six S, four sizes: WHOLE exactly where
    gzfile_serial_whole holds, LONG elsewhere, never OPEN."""
    t = equalities["verdict"]
    assert int(t[0]) > 1000000 and int(t[1]) == 0, t
    assert t[2::2] == ["whole", "long"] and all(int(x) > 0 for x in t[3::2]), t


def test_find_from_at_a_boundary_without_an_open_member(equalities):
    """in_len where the walk rested nowhere, else where it rested, and no OPEN stop."""
    t = equalities["from"]
    assert int(t[0]) == 100 and int(t[1]) == 0, t


def test_argument_checks(exe):
    got = dict(line.split() for line in subprocess.check_output([exe, "checks"]).decode().split("\n")[:-1])
    ok = {k for k, v in got.items() if v == "0"}
    assert ok == {"set_ok", "set_zero_ok", "set_largest_ok", "route_ok", "fresh_ok"}
    assert all(v == "-1" for k, v in got.items() if k not in ok) and len(got) == 15
