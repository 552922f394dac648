"""csrc/unit_discovery_rule.h without a GPU, through tests/host_model/unit_discovery_rule_model.cpp (built plainly and
with AddressSanitizer + UBSan, run as that program only).

The size rule: two counts fit one chain when their sum, taken without wrapping, is at most 0x7ffffff0 -- every pair
around the bound, around 2^31 and 2^32 - 1 (the counts saturate there), and zero on either side.  The carry's index: the
units of the last round, held against the round loop itself (u0 = 0, per_round, ... while u0 < n_dec), for every n_dec
up to 40 with every per_round up to 41, and at the 32-bit edge."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "unit_discovery_rule_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "unit_discovery_rule.h")]
EXE = os.path.join(HERE, "host_model", "unit_discovery_rule_model")
BOUND = 0x7FFFFFF0
U32 = 0xFFFFFFFF


def _build(out, extra):
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + extra + ["-I" + CSRC, SRC, "-o", out])
    return out


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request):
    if request.param == "plain":
        return _build(EXE, [])
    return _build(EXE + "_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run(exe, lines, tmp_path):
    p = tmp_path / "commands.txt"
    p.write_text("\n".join(lines) + "\n")
    out = subprocess.check_output([exe, "run", str(p)]).decode().split("\n")[:-1]
    assert len(out) == len(lines)
    return out


def test_size_rule(exe, tmp_path):
    edge = [0, 1, 2, 15, 16, 17, BOUND // 2, BOUND // 2 + 1, BOUND - 1, BOUND, BOUND + 1, 1 << 31, U32 - 1, U32]
    pairs = [(a, b) for a in edge for b in edge] + [(BOUND - k, k) for k in edge if k <= BOUND] + \
            [(BOUND - k + 1, k) for k in edge if k <= BOUND]
    want = ["1 %d" % (a + b) if a + b <= BOUND else "0 0" for a, b in pairs]
    assert run(exe, ["C %d %d" % p for p in pairs], tmp_path) == want
    assert "1 %d" % BOUND in want and "0 0" in want


def last_round(n_dec, per_round):
    count = 0
    for u0 in range(0, n_dec, per_round):  # the round driver's loop
        count = min(per_round, n_dec - u0)
    return count


def test_last_count(exe, tmp_path):
    cases = [(n, p) for n in range(1, 41) for p in range(1, 42)]
    want = ["%d" % last_round(n, p) for n, p in cases]
    # the 32-bit edge, where the loop cannot be run: n = q * p + r by hand
    big = [(U32, U32, U32), (U32, 1, 1), (U32, 4096, U32 % 4096), (1 << 31, 4096, 4096), (U32, U32 - 1, 1), (U32 - 1, U32, U32 - 1)]
    cases += [(n, p) for n, p, _ in big]
    want += ["%d" % r for _, _, r in big]
    assert run(exe, ["L %d %d" % c for c in cases], tmp_path) == want
