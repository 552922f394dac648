"""Where the pieces of grouped spliced streams lie, on the CPU: moonbit-flate_amd/csrc/splice_rule.h -- what the kernels
and the library's host code compile -- built with g++ into a stand-alone program under AddressSanitizer and UBSan (every
array in an allocation of exactly its size).  grouped_place must equal a plain walk over bit positions, one piece at a
time, for random maps with and without stored parts, every header and trailer length the containers have, groups of 1 ..
40 pieces and the piece counts around the chunk edges of a 1024-thread fold; `then` is associative; grouped_args_ok, the
grouped call's checks and zip_pieces_plan are tried on every refusal and with P around every entry length."""
import os
import random
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "splice_rule_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(CSRC, "splice_rule.h"), os.path.join(CSRC, "api_checks.h"), os.path.join(INC, "flate_hip.h")]
EXE = os.path.join(HERE, "host_model", "splice_rule_model")
NONE = (1 << 64) - 1
COUNTS = [1, 2, 1023, 1024, 1025, 2049, 5000]


def build():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + INC, SRC, "-o", EXE])
    return EXE


@pytest.fixture(scope="module")
def exe():
    return build()


def run(exe, mode, blob, tmp_path):
    args = [exe, mode]
    if blob is not None:
        path = tmp_path / (mode + ".bin")
        path.write_bytes(blob)
        args.append(str(path))
    out = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.splitlines()


def ints(s):
    return [int(x) for x in s.split()]


def align8(x):
    return (x + 7) & ~7


def step(x, a, b):
    """One piece: its bits in front of the first stored block (and that block's 3 header bits), the padding to a byte,
    everything behind."""
    x += a
    if b != NONE:
        x = align8(x) + b
    return x


def walk(maps, group_off, hdr, tl):
    """Bit positions, one piece at a time."""
    x = 0
    bit, end, pay, mem = [], [], [], []
    for g in range(len(group_off) - 1):
        mem.append(x // 8)
        x += 8 * hdr[g]
        pay.append(x // 8)
        for i in range(group_off[g], group_off[g + 1]):
            assert x % 8 == 0 or i > group_off[g]
            bit.append(x)
            x = step(x, *maps[i])
        end.append(x)
        x += 3            # BFINAL, BTYPE = 00
        x = align8(x)     # flush
        x += 32           # LEN, NLEN
        x += 8 * tl
    mem.append(x // 8)
    return x // 8, bit, end, pay, mem


def random_maps(rng, n, stored):
    maps = []
    for _ in range(n):
        a = rng.choice([0, 1, 7, 8, 9, rng.randrange(0, 600000)])
        b = NONE
        if stored and rng.random() < 0.4:
            b = rng.choice([32, 40, 32 + 8 * 65535, rng.randrange(0, 1 << 20)])
        maps.append((a, b))
    return maps


def random_groups(rng, n):
    off = [0]
    while off[-1] < n:
        off.append(min(n, off[-1] + rng.randint(1, 40)))
    return off


def place_cases():
    rng = random.Random(20260)
    cases = []
    for n in COUNTS:
        for stored in (False, True):
            for tl in (0, 4, 8):
                maps = random_maps(rng, n, stored)
                goff = random_groups(rng, n)
                g = len(goff) - 1
                for hdr in ([0] * g, [2] * g, [10] * g, [30 + rng.randint(1, 300) for _ in range(g)]):
                    cases.append((maps, goff, hdr, tl))
    # every piece its own group; one group of everything
    maps = random_maps(rng, 1025, True)
    cases.append((maps, list(range(1026)), [2] * 1025, 4))
    cases.append((maps, [0, 1025], [10], 8))
    return cases


def test_grouped_place_equals_the_walk(exe, tmp_path):
    cases = place_cases()
    blob = []
    for k, (maps, goff, hdr, tl) in enumerate(cases):
        n, g = len(maps), len(goff) - 1
        uniform = len(set(hdr)) == 1 and k % 2 == 0   # (the same length for every group: also without the array)
        blob.append(struct.pack("<5I", n, g, tl, 0 if uniform else 1, hdr[0] if uniform else 0xdead))
        blob.append(struct.pack("<%dQ" % (2 * n), *[v for m in maps for v in m]))
        blob.append(struct.pack("<%dI" % (g + 1), *goff))
        if not uniform:
            blob.append(struct.pack("<%dI" % g, *hdr))
    rows = run(exe, "place", b"".join(blob), tmp_path)
    assert len(rows) == len(cases)
    for (maps, goff, hdr, tl), ln in zip(cases, rows):
        total, bit, end, pay, mem = walk(maps, goff, hdr, tl)
        parts = ln.split("|")
        assert int(parts[0]) == total
        assert ints(parts[1]) == bit and ints(parts[2]) == end and ints(parts[3]) == pay and ints(parts[4]) == mem


def test_then_is_associative_and_composes_apply(exe, tmp_path):
    rng = random.Random(7)

    def m():
        a = rng.choice([0, 3, rng.randrange(0, 1 << 40)])
        return a, (NONE if rng.random() < 0.5 else rng.choice([0, 32, rng.randrange(0, 1 << 40)]))

    triples = [(m(), m(), m(), rng.choice([0, 1, 7, 8, rng.randrange(0, 1 << 40)])) for _ in range(10000)]
    blob = b"".join(struct.pack("<7Q", f[0], f[1], g[0], g[1], h[0], h[1], x) for f, g, h, x in triples)
    rows = run(exe, "assoc", blob, tmp_path)
    assert len(rows) == len(triples)
    for (f, g, h, x), ln in zip(triples, rows):
        la, lb, ma, mb, serial, composed = ints(ln)
        assert (la, lb) == (ma, mb), (f, g, h)
        assert serial == composed == step(step(step(x, *f), *g), *h), (f, g, h, x)


def test_grouped_args_ok(exe, tmp_path):
    cases = [([0, 1], 1, 1), ([0, 3], 3, 1), ([0, 1, 2, 3], 3, 1), ([0, 2, 3], 3, 1), ([0], 0, 1),
             ([0, 0], 0, 0), ([0, 1, 1], 1, 0), ([0, 2, 1], 1, 0), ([1, 2], 2, 0), ([0, 2], 3, 0), ([0, 4], 3, 0),
             ([0], 1, 0), ([0, 3, 2, 5], 5, 0), ([0, 0xffffffff], 0xffffffff, 1), ([0, 5, 5], 5, 0)]
    blob = b"".join(struct.pack("<2I", len(g) - 1, n) + struct.pack("<%dI" % len(g), *g) for g, n, _ in cases)
    assert [int(x) for x in run(exe, "args", blob, tmp_path)] == [ok for _, _, ok in cases]


def test_the_grouped_calls_refusals(exe, tmp_path):
    assert [int(x) for x in run(exe, "api", None, tmp_path)] == [0, 0, 0, 0] + [-1] * 13


def plan(in_off, P):
    pin, goff, longs = [], [0], 0
    for lo, hi in zip(in_off, in_off[1:]):
        if P >= 1 and hi - lo > P:
            pin += list(range(lo, hi, P))
            longs += 1
        else:
            pin.append(lo)
        goff.append(len(pin))
    return len(pin), longs, pin + [in_off[-1]], goff


def test_zip_pieces_plan_with_p_around_every_entry_length(exe, tmp_path):
    lens = [0, 5, 300, 3000, 70000, 200000, 1, 65535, 65536]
    in_off = [7]
    for n in lens:
        in_off.append(in_off[-1] + n)
    sizes = {0, 1, 2, 1000, 4096, 1 << 40}
    for n in lens:
        sizes |= {max(n - 1, 0), n, n + 1, n // 2, n // 2 + 1, n // 3 + 1}
    cases = [(in_off, P) for P in sorted(sizes)] + [([0], 5), ([3], 0), ([0, 0], 1), ([0, 10], 1)]
    blob = b"".join(struct.pack("<IQ", len(o) - 1, P) + struct.pack("<%dQ" % len(o), *o) for o, P in cases)
    rows = run(exe, "plan", blob, tmp_path)
    assert len(rows) == len(cases)
    for (o, P), ln in zip(cases, rows):
        count, longs, pin, goff = plan(o, P)
        head, a, b = ln.split("|")
        assert ints(head) == [count, longs], (o, P)
        assert ints(a) == pin and ints(b) == goff, (o, P)
        # the pieces tile the input, none is longer than P where P is on, every long entry is ceil(len / P) pieces
        assert pin == sorted(pin) and pin[0] == o[0] and pin[-1] == o[-1]
        if P >= 1:
            for g, (lo, hi) in enumerate(zip(o, o[1:])):
                k = goff[g + 1] - goff[g]
                assert k == (max(1, -(-(hi - lo) // P)))
                assert all(pin[i + 1] - pin[i] <= max(P, 0) or k == 1 for i in range(goff[g], goff[g + 1]))
