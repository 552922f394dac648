"""The rule of ONE stream written in parts on the CPU: moonbit-flate_amd/csrc/one_writer_rule.h -- the functions the
writer's kernels and flate_hip_one_writer_write compile -- and api_checks.h's one_writer_*_check, built with g++ into a
stand-alone program (once plainly, once under AddressSanitizer and UBSan; both run as that program only) and compared
with the Python reference tests/one_writer_ref.py: every call's status, in_used, out_len, n_pieces, header, close, start
bit and carry, for P in {1, 17, 300}, T in {0, 1, P - 1, P, P + 1, 3P, 3P + 5}, every position of the first cut, every
out_cap from 0 to the bytes needed, and every carry 0..7."""
import os
import subprocess

import numpy as np
import pytest

import one_writer_ref as R
from util import make_streams

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "one_writer_rule_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(INC, "flate_hip.h")] + [os.path.join(CSRC, h) for h in ("one_writer_rule.h", "api_checks.h")]
EXE = os.path.join(HERE, "host_model", "one_writer_rule_model")
PIECES = (1, 17, 300)


def totals(P):
    return sorted({0, 1, P - 1, P, P + 1, 3 * P, 3 * P + 5})


def _build(out, extra):
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + extra + ["-I" + CSRC, "-I" + INC, SRC, "-o", out])
    return out


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request):
    if request.param == "plain":
        return _build(EXE, [])
    return _build(EXE + "_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run(exe, lines, tmp_path):
    p = tmp_path / "commands.txt"
    p.write_text("\n".join(lines) + "\n")
    return subprocess.check_output([exe, "run", str(p)]).decode().split("\n")[:-1]


@pytest.fixture(scope="module")
def wholes(oracle):
    """{(P, T, wrap): Whole}: text with runs of random bytes in it (stored blocks: the align8 branch), every stream from
    another place of it so that the ends of the pieces fall on every bit of a byte; computed once, shared, never
    changed."""
    data, _ = make_streams([("text", 400), ("rand", 200), ("text", 200), ("zero", 60), ("rand", 45), ("text", 400)], seed=21)
    data = data.tobytes()
    out = {}
    for P in PIECES:
        for k, T in enumerate(totals(P)):
            for wrap in (R.RAW, R.ZLIB, R.GZIP):
                out[(P, T, wrap)] = R.Whole(oracle, data[37 * k + 11 * wrap:][:T], P, wrap, "go" if (k + wrap) % 2 else "moonbit")
    return out


def line_of(c, carry_before, fits=True):
    if c.n_pieces == 0 and not c.final:
        return "0 0 0 0 0 0 0 %d" % carry_before
    if not fits:
        return "%d 0 %d 0 %d %d %d %d" % (R.E_OUT_TOO_SMALL, c.out_len, c.header, c.close, c.start_bit, carry_before)
    return "%d %d %d %d %d %d %d %d" % (c.rc, c.in_used, c.out_len, c.n_pieces, c.header, c.close, c.start_bit, c.carry)


def script(w, sizes, all_caps, calls=None):
    """The commands of one writer over the part list, and the lines the reference expects: every call first with every
    capacity below the bytes it needs (all_caps; else with one byte too few), then with exactly enough; one more write
    behind the end."""
    lines, want, carry = ["N %d %d" % (w.wrap, w.piece)], ["ok"], 0
    for c in calls or w.calls(sizes):
        launches = c.n_pieces or c.final
        caps = (range(c.out_len) if all_caps else [c.out_len - 1] if c.out_len else []) if launches else []
        for cap in caps:
            lines.append("W %d %d %d %d" % (c.in_len, c.final, cap, c.span))
            want.append(line_of(c, carry, fits=False))
        lines.append("W %d %d %d %d" % (c.in_len, c.final, c.out_len, c.span))
        want.append(line_of(c, carry))
        if launches:
            carry = c.carry
    lines.append("W 5 0 100 40")
    want.append("%d 0 0 0 0 0 0 0" % R.E_INVALID)
    return lines, want


@pytest.fixture(scope="module")
def first_cuts(wholes):
    """(commands, expected lines, the carries seen) of every first cut: made once for both builds of the program."""
    lines, want, carries = [], [], set()
    for (P, T, wrap), w in wholes.items():
        for cut in range(T + 1):
            # a first call with `cut` bytes, a second with P more, the final one with the rest
            calls = w.calls([cut, P])
            l, x = script(w, [cut, P], all_caps=True, calls=calls)
            lines += l
            want += x
            carries |= {c.carry for c in calls if c.carry is not None and not c.final}
    return lines, want, carries


def test_every_first_cut_and_every_capacity(exe, tmp_path, first_cuts):
    lines, want, carries = first_cuts
    assert carries == set(range(8)), carries  # (from the oracle's index: every carry stands at some call's end)
    got = run(exe, lines, tmp_path)
    assert len(got) == len(want)
    bad = [(i, lines[i], g, x) for i, (g, x) in enumerate(zip(got, want)) if g != x]
    assert not bad, bad[:3]


def test_part_lists(exe, tmp_path, wholes):
    lines, want = [], []
    for (P, T, wrap), w in wholes.items():
        for sizes in ([], R.fixed(T, 1), R.fixed(T, P), R.fixed(T, P - 1), R.fixed(T, 2 * P + 1), R.growing(T),
                      R.random_sizes(T, P, seed=P + T), [0, 0, T, 0]):
            l, x = script(w, sizes, all_caps=False)
            lines += l
            want += x
    assert run(exe, lines, tmp_path) == want


def test_the_end_at_every_carry(exe, tmp_path):
    """one_writer_end for every bit phase: whole bytes, carry, the bytes needed against every capacity around them."""
    lines, want = [], []
    for wrap in (R.RAW, R.ZLIB, R.GZIP):
        for end_bit in list(range(0, 64)) + [8 * 10 + b for b in range(8)] + [(1 << 40) + b for b in range(8)]:
            for close in (0, 1):
                whole = (end_bit + 3 + 7) // 8 + 4 + R.TRAILER[wrap] if close else end_bit // 8
                for cap in {0, max(whole - 1, 0), whole, whole + 1}:
                    lines.append("E %d %d %d %d" % (end_bit, close, wrap, cap))
                    want.append("%d %d %d" % (whole, 0 if close else end_bit % 8, int(whole <= cap)))
    assert run(exe, lines, tmp_path) == want


def test_limits_and_arguments(exe, tmp_path):
    lines = ["N 2 0", "W %d 0 0 0" % (1 << 32), "W %d 1 0 0" % (1 << 32), "W 65534 0 0 0",
             # open: ctx wrap P flags writer
             "O 1 2 0 0 1", "O 1 0 65535 3 1", "O 0 2 0 0 1", "O 1 2 0 0 0", "O 1 3 0 0 1", "O 1 2 %d 0 1" % 0x7ffe0000,
             "O 1 2 %d 0 1" % 0x7ffdffff, "O 1 2 0 4 1", "O 1 2 0 8 1",
             # write: w in in_len out out_cap used len np
             "A 1 1 5 1 9 1 1 1", "A 0 1 5 1 9 1 1 1", "A 1 0 5 1 9 1 1 1", "A 1 0 0 1 9 1 1 1", "A 1 1 5 0 9 1 1 1",
             "A 1 1 5 0 0 1 1 1", "A 1 1 5 1 9 0 1 1", "A 1 1 5 1 9 1 0 1", "A 1 1 5 1 9 1 1 0"]
    want = ["ok", "-6 0 0 0 0 0 0 0", "-6 0 0 0 0 0 0 0", "0 0 0 0 0 0 0 0",
            "0", "0", "-1", "-1", "-1", "-1", "0", "-1", "-1",
            "0", "-1", "-1", "0", "-1", "0", "-1", "-1", "-1"]
    assert run(exe, lines, tmp_path) == want


def test_the_bound(exe, tmp_path, wholes):
    """Monotone in in_len, the reference's formula, and at least the largest call of the corpus."""
    lines = ["B %d %d" % (n, P) for P in (0,) + PIECES for n in range(0, 2000, 7)]
    got = [int(x) for x in run(exe, lines, tmp_path)]
    want = [R.bound(n, P) for P in (0,) + PIECES for n in range(0, 2000, 7)]
    assert got == want
    per = len(range(0, 2000, 7))
    for k in range(4):
        assert np.all(np.diff(got[k * per:(k + 1) * per]) >= 0)
    for (P, T, wrap), w in wholes.items():
        for sizes in ([], [T], R.fixed(T, P), [1, P]):
            for c in w.calls(sizes):
                assert c.out_len <= R.bound(c.in_len, P), (P, T, wrap, c)
