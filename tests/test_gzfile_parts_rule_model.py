"""The rule of a gzip FILE read in parts on the CPU: moonbit-flate_amd/csrc/gzfile_parts_rule.h -- the functions the part
kernels and flate_hip_gzfile_reader_read compile -- and api_checks.h's gzfile_reader_*_args, built with g++ into a
stand-alone program under AddressSanitizer and UBSan and compared with the Python reference tests/gzfile_parts_ref.py:
THE PARTS HOP at every cut of a trailer plus a header with FEXTRA, FNAME, FCOMMENT and FHCRC, final and not, and whole
readers -- every call's eight words -- at every cut position of two small files, with small capacities, with wrong
trailers, truncated and corrupt files, bytes behind the last member, and a wrong trailer in front of a corrupt member.
The program holds one_parts_header against gzip_header_len on every header it sees."""
import os
import subprocess

import pytest

import gzfile_parts_ref as R
import gzfile_ref as gf
import gzip_ref as gz
import one_parts_ref as opr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "gzfile_parts_rule_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(INC, "flate_hip.h")] + [os.path.join(CSRC, h) for h in (
    "gzfile_parts_rule.h", "gzfile_rule.h", "one_parts_rule.h", "api_checks.h", "gzip_rule.h")]
EXE = os.path.join(HERE, "host_model", "gzfile_parts_rule_model")
END, DEAD, NEXT, STOP = 0, 1, 2, 3


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


def hexs(b):
    return bytes(b).hex() or "-"


# ---- the parts hop ----

def hop_ref(buf, b, final):
    """THE PARTS HOP from gzfile_ref.hop and one_parts_ref.header_state."""
    kind, e, bit = gf.hop(buf, b)
    if final:
        return {"end": END, "dead": DEAD, "next": NEXT}[kind], e, bit
    if kind == "next":
        return NEXT, e, bit
    if e >= len(buf):
        return (STOP if e == len(buf) else DEAD), e, 0
    return (DEAD if opr.header_state(opr.GZIP, buf[e:])[0] == opr.BAD else STOP), e, 0


def test_the_hop_at_every_cut_of_a_trailer_and_a_header(exe, tmp_path):
    t = gz.text(400, seed=3)
    first = gz.member(t[:200], 6)
    second = gz.member(t[200:], 6, flg=gz.FEXTRA | gz.FNAME | gz.FCOMMENT | gz.FHCRC, extra=b"ab\x03\x00xyz", name=b"a name",
                       comment=b"a comment")
    f = first + second
    w = gf.Walk(f)
    b = w.end_bits[0]
    hdr = w.unit_bit[w.member_unit[1]] // 8 - len(first)
    assert hdr == 10 + 2 + 7 + 7 + 10 + 2
    lines, want = [], []
    damaged = bytearray(f)
    damaged[len(first) + 12] ^= 0  # (the same bytes; the damage below is in the fixed part)
    for buf in (f, bytes(f[:len(first)] + b"\x1f\x8b\x07" + f[len(first) + 3:]), bytes(f[:len(first) + 3] + b"\xe0" + f[len(first) + 4:])):
        for cut in range(len(first), len(first) + hdr + 12):
            for final in (0, 1):
                lines.append("P %d %d %s" % (final, b, hexs(buf[:cut])))
                want.append("%d %d %d" % hop_ref(buf[:cut], b, final))
    got = run(exe, lines, tmp_path)
    assert got == want, [(i, g, x) for i, (g, x) in enumerate(zip(got, want)) if g != x][:3]
    assert {x.split()[0] for x in want} == {"0", "1", "2", "3"}  # every answer occurs


# ---- whole readers ----

def world(m):
    """The `F`, `W` and `T` lines of a Model: the walk over the whole file as the program takes it."""
    w, n = m.w, m.w.n_units
    unit_fail = w.status != 0 and len(m.member_of) > n  # the walk fails IN a unit (not where a header had to stand)
    members = w.n_members + (1 if unit_fail else 0)
    start = [0] * (n + 1)
    for j in range(members):
        if w.member_unit[j] <= n:
            start[w.member_unit[j]] = w.member_off[j] + 1
    fin, end = [], []
    for k in range(n):
        j = m.member_of[k]
        last = j < w.n_members and (k + 1 == len(m.member_of) or m.member_of[k + 1] != j)
        fin.append(int(last))
        end.append(w.end_bits[j] if last else w.unit_bit[k + 1])
    fail_raw = w.unit_bit[w.member_unit[w.bad_member]] // 8 if unit_fail else 0
    words = [n, w.status if unit_fail else 0, fail_raw, w.stream_err_off if unit_fail else -1,
             w.out_len - w.out_off[n] if unit_fail else 0]
    words += w.unit_bit[:n + 1] + w.out_off[:n + 1] + start + m.reach + end + fin
    ok = [int(m._trailer_ok(j)) for j in range(w.n_members)]
    return ["F " + hexs(m.f), "W " + " ".join(map(str, words)), "T %d %s" % (len(ok), " ".join(map(str, ok)))]


class Recorded:
    def __init__(self, m):
        self.m, self.lines, self.expect = m, world(m), []

    def fresh(self):
        self.m.reset()
        self.lines.append("N %d" % self.m.unit_max)
        self.model_read = R.model_reader(self.m)

    def read(self, buf, final, out_cap):
        self.lines.append("R %d %d %d" % (len(buf), final, out_cap if out_cap is not None else 1 << 62))
        c, got = self.model_read(buf, final, out_cap)
        self.expect.append(c)
        return c, got

    def check(self, exe, tmp_path, what):
        got = run(exe, self.lines, tmp_path)
        want = ["%d %d %d %d %d %d %d %d" % c for c in self.expect]
        assert got == want, (what, [(i, g, x) for i, (g, x) in enumerate(zip(got, want)) if g != x][:3])


def files():
    three = b"".join(x for x, _ in gf.three_members())
    return [("three_members", three), ("tiny_file", gf.tiny_file()[0])]


@pytest.mark.parametrize("what,f", files(), ids=[x for x, _ in files()])
def test_whole_readers_at_every_cut(exe, tmp_path, what, f):
    plain = b"".join(gf.members_of(f))
    rec = Recorded(R.Model(f))
    for cut in range(0, len(f) + 1):
        rec.fresh()
        calls, out, rest = R.feed(rec.read, f, [cut], None, 8, grow=len(f))
        assert calls[-1].rc == R.STREAM_END and out == plain and not rest, cut
    for cap, step in ((1, 700), (300, 64), (1500, 1000), (4096, 333)):
        rec.fresh()
        calls, out, rest = R.feed(rec.read, f, iter(lambda: step, 0), cap, 4000, grow=step)
        assert plain.startswith(out) and calls[-1].rc in (R.STREAM_END, R.OUT_TOO_SMALL)
    rec.check(exe, tmp_path, what)


def failing_files():
    three = gf.three_members()
    f = b"".join(x for x, _ in three)
    plain = b"".join(p for _, p in three)
    w = gf.Walk(f)
    out = []
    for k in range(3):
        for what, at, bit in (("CRC-32", -8, 0x40), ("ISIZE", -4, 0x01)):
            bad = bytearray(f)
            bad[w.member_off[k + 1] + at] ^= bit
            out.append(("a wrong %s in member %d" % (what, k), bytes(bad)))
    a, ab = w.member_off[1], w.member_off[2]
    out.append(("cut inside the last member's stream", f[:ab + (len(f) - ab) // 2]))
    out.append(("cut inside the last member's trailer", f[:-3]))
    out.append(("cut inside the middle member's header", f[:a + 7]))
    u = w.member_unit[1] + 2
    bad = bytearray(f)
    bit = w.unit_bit[u] + 1  # BTYPE = 2 -> 3
    bad[bit >> 3] |= 1 << (bit & 7)
    out.append(("a corrupt middle member", bytes(bad)))
    out.append(("zero bytes behind the last member", f + b"\0" * 8))
    out.append(("garbage behind the last member", f + b"garbage, and more of it"))
    bad[w.member_off[1] - 8] ^= 1
    out.append(("a wrong trailer in front of a corrupt member", bytes(bad)))
    return plain, out


@pytest.mark.parametrize("case", failing_files()[1], ids=[x for x, _ in failing_files()[1]])
def test_failing_files(exe, tmp_path, case):
    what, f = case
    plain = failing_files()[0]
    m = R.Model(f, plain=plain)
    rec = Recorded(m)
    ends = set()
    for cut in list(range(0, len(f) + 1, 7)) + [len(f)]:
        rec.fresh()
        calls, out, rest = R.feed(rec.read, f, [cut], None, 8, grow=len(f))
        c = calls[-1]
        assert c.rc < 0 and c.in_used == 0 and plain.startswith(out), (what, cut)
        ends.add((c.rc, c.bad_member, c.err_off, c.stream_err_off, len(out)))
    assert len(ends) == 1, (what, ends)  # the same answer for every cut
    w = m.w
    if "in front of" in what:  # the documented difference: the reader reports the trailer, the walk the break
        assert ends == {(R.CORRUPT, 0, 0, w.member_off[1], w.out_off[w.member_unit[1]])}
        assert (w.status, w.bad_member) == (R.CORRUPT, 1)
    elif "wrong" in what:
        (rc, bad, eo, so, n), = ends
        assert (rc, eo, so, n) == (R.CORRUPT, w.member_off[bad], w.member_off[bad + 1] - w.member_off[bad],
                                   w.out_off[w.member_unit[bad + 1]])
    else:
        assert ends == {(w.status, w.bad_member, w.err_off, w.stream_err_off, w.out_len)}
    rec.check(exe, tmp_path, what)


def test_argument_checks(exe):
    got = dict(line.split() for line in subprocess.check_output([exe, "checks"]).decode().split("\n")[:-1])
    ok = {k for k, v in got.items() if v == "0"}
    assert ok == {"open_ok", "open_device_ok", "read_ok", "read_nothing_ok"}
    assert all(v == "-1" for k, v in got.items() if k not in ok) and len(got) == 13
