"""The rule of ZIP's long entries on the CPU: moonbit-flate_amd/csrc/zip_units_rule.h -- the functions the kernels and
the library's host code compile -- built with g++ into a stand-alone program under AddressSanitizer and UBSan and
compared with tests/zip_units_ref.py, the restatement over zip_ref.Index, one_ref.Walk and stored_ref.Walk: the set L
for thresholds around every entry's comp_size, duplicates, overlapping ranges and chain order against file order; every
node's link, the units of the path, their slots and history lengths, and g.  The same program drives zip_unit_min_ok."""
import os
import struct
import subprocess
import zlib

import pytest

import gzip_ref
import one_ref
import zip_ref as ref
import zip_units_ref as zu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "zip_units_rule_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(CSRC, "zip_units_rule.h"), os.path.join(CSRC, "chain_rule.h"), os.path.join(CSRC, "api_checks.h"),
        os.path.join(INC, "flate_hip.h")]
EXE = os.path.join(HERE, "host_model", "zip_units_rule_model")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + INC, SRC, "-o", EXE])
    return EXE


def run(exe, mode, blob, tmp_path):
    path = tmp_path / (mode + ".bin")
    path.write_bytes(blob)
    return subprocess.run([exe, mode, str(path)], check=True, capture_output=True, text=True).stdout.splitlines()


def archive_of(items):
    f, _ = ref.write_archive([r for r, _ in items], [b"n%d" % k for k in range(len(items))],
                             [zlib.crc32(p) for _, p in items], [len(p) for _, p in items])
    return f


def long_archives():
    """(what, archive): the streams of the GPU tests' archives, smaller."""
    t = gzip_ref.text(60000, seed=21)
    r = gzip_ref.rand(70000, seed=8)
    mixed = t[:20000] + r + t[20000:40000]
    many = (one_ref.deflate(t, 6, mem=1), t)
    l6 = (one_ref.deflate(t, 6), t)
    rnd = (one_ref.deflate(r, 6), r)
    mix = (one_ref.deflate(mixed, 6), mixed)
    one = (one_ref.deflate(t[:5000], 9), t[:5000])
    empty = (one_ref.deflate(b"", 6), b"")
    assert one_ref.Walk(many[0]).n_units >= 8
    base = archive_of([one, many, l6])
    ix = ref.Index(base)
    rec = [e.name_off - 46 for e in ix.entries]
    e1 = ix.entries[1]
    two = archive_of([many, many, one])
    jx = ref.Index(two)
    two = ref._patch(two, jx.entries[1].name_off - 46 + 42, "<I", jx.entries[0].header_off)
    # a record whose range starts inside another entry's data
    inside = ref._patch(base, rec[2] + 42, "<I", ix.entries[1].header_off + 7)
    return [
        ("the streams", archive_of([many, l6, rnd, empty, mix, one])),
        ("a stream cut short", ref._patch(base, rec[1] + 20, "<I", e1.comp_size - 3)),
        ("a size too small", ref._patch(base, rec[1] + 24, "<I", e1.size - 1)),
        ("a size too large", ref._patch(base, rec[1] + 24, "<I", e1.size + 1)),
        ("BFINAL in front of comp_size", archive_of([one, (many[0] + gzip_ref.rand(500, seed=3), t), l6])),
        ("two records over the same data", two),
        ("a record inside another's data", inside),
    ]


def all_archives():
    out = [(w, f) for w, f in ref.zipfile_corpus(big=False)]
    out += [(w, f) for k, (w, f) in enumerate(ref.hostile_corpus()) if not (w.startswith("truncated") and k % 13)]
    out += [(w, f) for w, f, _, _, _ in ref.entry_cases()]
    return out + long_archives()


def selections(n):
    if n == 0:
        return [None]
    return [None, list(range(n))[::-1], [0, n - 1, 0, n // 2, 0][:n + 2], list(range(0, n, 2))]


def test_the_set_L_equals_the_reference(exe, tmp_path):
    cases, blob = [], []
    for what, f in all_archives():
        ix = ref.Index(f)
        if ix.rc != 0:
            continue
        sizes = sorted({e.comp_size for e in ix.entries if e.method == 8})
        mins = sorted({0, 1} | {s + d for s in sizes for d in (0, 1)})
        for sel in selections(ix.n_entries):
            for v in mins:
                cases.append((what, ix, sel, v))
                b = struct.pack("<QI", v, ix.n_entries)
                b += b"".join(struct.pack("<QQQiI", e.data_off, e.comp_size, e.size, e.status, e.method) for e in ix.entries)
                b += struct.pack("<II", 0 if sel is None else 1, 0 if sel is None else len(sel))
                b += b"".join(struct.pack("<I", s) for s in (sel or []))
                blob.append(b)
    lines = run(exe, "form", struct.pack("<I", len(blob)) + b"".join(blob), tmp_path)
    assert len(lines) == len(cases)
    some_dup = some_overlap = some_order = False
    for (what, ix, sel, v), line in zip(cases, lines):
        head, ls, rs = [p.split() for p in line.split("|")]
        L, fallback, (lo, hi) = zu.form(ix.entries, sel, v)
        assert [int(x) for x in head] == [fallback, lo, hi], (what, sel, v)
        want = [(c["slot"], c["lo"] - lo, c["end"] - lo, c["size"], c["out"]) for c in L]
        assert [tuple(int(x) for x in e.split(",")) for e in ls] == want, (what, sel, v)
        got_r = [tuple(int(x) for x in e.split(",")) for e in rs]
        assert got_r == sorted((c["lo"] - lo, c["end"] - lo, k) for k, c in enumerate(L)), (what, sel, v)
        some_dup |= fallback > 0 and sel is not None
        some_overlap |= fallback > 0 and sel is None
        some_order |= [r[2] for r in got_r] != sorted(r[2] for r in got_r)
        if v == 0:
            assert not L and fallback == 0
    assert some_dup and some_overlap and some_order


def chain_blob(c, L, lo0):
    b = struct.pack("<II", len(c["cand"]), len(L)) + b"".join(struct.pack("<Q", x) for x in c["cand"])
    b += b"".join(struct.pack("<QQQQ", e["lo"] - lo0, e["end"] - lo0, e["size"], e["out"]) for e in L)
    return b + b"".join(struct.pack("<IIQQ", *p) for p in c["probes"])


def test_links_units_slots_and_g_equal_the_reference(exe, tmp_path):
    cases, blob = [], []
    for what, f in long_archives() + [(w, f) for w, f, _, _, _ in ref.entry_cases()]:
        ix = ref.Index(f)
        for sel in (None, list(range(ix.n_entries))[::-1]):
            for stored in (False, True):
                L, _, hull = zu.form(ix.entries, sel, 1)
                if not L:
                    continue
                # decoys: a bit inside no range (a local header between two entries), one inside a range off the path
                decoys = {8 * (c["end"] - hull[0]) + 3 for c in L if c["end"] < hull[1]}
                decoys |= {8 * (L[0]["lo"] - hull[0]) + 1}
                c = zu.chain(f, L, hull, stored, decoys)
                cases.append((what, sel, stored, c, L))
                blob.append(chain_blob(c, L, hull[0]))
    lines = run(exe, "chain", struct.pack("<I", len(blob)) + b"".join(blob), tmp_path)
    assert len(lines) == len(cases)
    gs = set()
    for (what, sel, stored, c, L), line in zip(cases, lines):
        nxt, units, g = [p.split() for p in line.split("|")]
        assert [int(x) for x in nxt] == c["next"], (what, sel, stored)
        assert [tuple(int(x) for x in u.split(",")) for u in units] == c["units"], (what, sel, stored)
        assert int(g[0]) == c["g"], (what, sel, stored)
        gs.add((what, c["g"], len(L)))
        assert all(h == min(32768, s - L[x]["out"]) for _, x, s, h in c["units"])
    by = {(w, g == n) for w, g, n in gs}
    assert ("the streams", True) in by and ("a stream cut short", False) in by and ("a size too small", False) in by
    assert ("BFINAL in front of comp_size", True) in by


def test_served_entries(exe, tmp_path):
    cases = [(3, 0xffffffff, [0, 4, 5, 9]), (3, 9, [0, 4, 5, 9]), (3, 8, [0, 4, 5, 9]), (3, 4, [0, 4, 5, 9]),
             (3, 0, [0, 4, 5, 9]), (1, 0, [0, 1]), (0, 0xffffffff, [0]), (2, 5, [0, 5, 5])]
    blob = struct.pack("<I", len(cases)) + b"".join(
        struct.pack("<II", g, bad) + b"".join(struct.pack("<Q", u) for u in eu) for g, bad, eu in cases)
    got = [int(x) for x in run(exe, "served", blob, tmp_path)]
    assert got == [zu.served(eu, g, bad) for g, bad, eu in cases] == [3, 3, 2, 1, 0, 0, 0, 2]


def test_zip_unit_min_ok(exe):
    lines = subprocess.run([exe, "checks"], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {int(a): int(b) for a, b in (ln.split() for ln in lines if ln)}
    assert got == {-1: 0, 0: 1, 1: 1, 2: 1, 65536: 1, 1 << 40: 1, (1 << 63) - 1: 1, -(1 << 63): 0}
