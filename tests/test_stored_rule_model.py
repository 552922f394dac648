"""The stored-header rule of the option "one_stored_units" on the CPU: deflate_stored_header_ok of
moonbit-flate_amd/csrc/deflate_block_rule.h -- what the discovery kernels compile -- built with g++ into a stand-alone
program under AddressSanitizer and UBSan, run at EVERY bit offset of the corpus streams (each in an allocation of exactly
its size) and compared with the restatement in tests/stored_ref.py.  Every stored header the walker reaches must be a
hit, whatever its padding bits hold.  The same program drives one_stored_units_ok and the check of a seek index's rule
word; stored_ref.Walk itself is held against one_ref.Walk."""
import os
import struct
import subprocess

import pytest

import deflate_corpus as dc
import one_ref
import stored_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "deflate_stored_rule_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(INC, "flate_hip.h")] + [os.path.join(CSRC, h) for h in (
    "deflate_block_rule.h", "api_checks.h", "seek_index_rule.h", "gzfile_seek_rule.h", "bgzf_range_rule.h")]
EXE = os.path.join(HERE, "host_model", "deflate_stored_rule_model")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + INC, SRC, "-o", EXE])
    return EXE


@pytest.fixture(scope="module")
def good():
    """[(what, raw stream, plain)] of one_ref: computed once."""
    return one_ref.good_streams()


def header_cases():
    """[(what, stream)]: stored headers built by hand at every bit phase, with ones as padding."""
    out = []
    for phase in range(8):
        for what, kw, tail in (("LEN = 7", {}, b""), ("LEN = 0", {"payload": b""}, b""),
                               ("NLEN off by one bit", {"nlength": (~7 & 0xffff) ^ 0x0400}, b""),
                               ("LEN off by one bit", {"length": 7 ^ 0x0001, "nlength": ~7 & 0xffff}, b"")):
            w = dc.Writer()
            dc.prefix_block(w, phase)
            ref.stored_block(w, kw.pop("payload", b"payload"), final=True, **kw)
            out.append(("phase %d, %s" % (phase, what), w.data()))
        # the header in the stream's last bytes: 3 and then 4 bytes behind q, and q behind the last byte
        w = dc.Writer()
        dc.prefix_block(w, phase)
        ref.stored_block(w, b"", final=True)
        whole = w.data()
        out += [("phase %d, %d bytes behind q" % (phase, 4 - cut), whole[:len(whole) - cut]) for cut in (0, 1, 2, 3, 4)]
    return out


def run(exe, tmp_path, cases):
    """cases: [stream] -> per case the bit offsets (all of them, and eight behind the end) at which the C++ rule holds."""
    blob = [struct.pack("<I", len(cases))]
    for raw in cases:
        blob.append(struct.pack("<Q", len(raw)) + raw + struct.pack("<Q", 0))
    path = tmp_path / "cases.bin"
    path.write_bytes(b"".join(blob))
    lines = subprocess.run([exe, "rule", str(path)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert len(lines) == len(cases) + 1
    return [[int(x) for x in line.split()] for line in lines[:-1]]


def test_rule_equals_the_python_reference_at_every_bit(exe, good, tmp_path):
    streams = [(w, r) for w, r, _ in good + one_ref.decoy_streams()]
    streams += [(w, r) for w, r, _, _ in ref.hand_streams()] + [(w, r) for w, r, _ in ref.failing_streams()]
    streams += header_cases()
    got = run(exe, tmp_path, [r for _, r in streams])
    for (what, raw), g in zip(streams, got):
        assert g == ref.hits(raw), what
        if len(raw) <= 3000:  # the rule itself at every offset, the eight behind the end included
            assert g == [b for b in range(8 * len(raw) + 8) if ref.rule(raw, b)], what
        # every stored header the serial decode reaches whole is a hit, or the chain has holes
        assert {b[0] for b in ref.Walk(raw).blocks if b[1] == 0} <= set(g), what


def test_hand_built_headers(exe, tmp_path):
    cases = header_cases()
    got = dict(zip((w for w, _ in cases), run(exe, tmp_path, [r for _, r in cases])))
    for phase in range(8):
        w = dc.Writer()
        dc.prefix_block(w, phase)
        at = w.pos
        assert at % 8 == phase
        assert at in got["phase %d, LEN = 7" % phase] and at in got["phase %d, LEN = 0" % phase]
        assert got["phase %d, NLEN off by one bit" % phase] == [] and got["phase %d, LEN off by one bit" % phase] == []
        assert at in got["phase %d, 4 bytes behind q" % phase]
        for k in (3, 2, 1, 0):
            assert got["phase %d, %d bytes behind q" % (phase, k)] == []
        # up to 8 offsets in front of ONE pair pass, all of them with the same q; the padding bits were ones
        hits = got["phase %d, LEN = 0" % phase]
        assert 1 <= len(hits) <= 8 and len({(b + 10) // 8 for b in hits}) == 1


def test_counts_of_the_issue(good):
    by = {w: r for w, r, _ in good}
    for what, raw in by.items():
        w = ref.Walk(raw)
        assert {b[0] for b in w.blocks if b[1] == 0} <= set(ref.hits(raw)), what
    level0 = by["level 0 only: one unit"]
    assert [b[1] for b in ref.Walk(level0).blocks] == [0] * 4 and len(ref.hits(level0)) == 28
    flush = by["Z_FULL_FLUSH every 10 000 bytes: empty stored blocks inside units"]
    assert sum(1 for b in ref.Walk(flush).blocks if b[1] == 0) == 30 and len(ref.hits(flush)) == 188
    import gzip_ref
    r = one_ref.deflate(gzip_ref.rand(300000, seed=8), 6)
    # 300 000 random bytes (gzip_ref.rand, seed 8) at level 6: 19 stored blocks of about 16 390 bytes and exactly 149
    # passing offsets.  (The issue's 140 came from other random bytes: the count depends on how many of the up to 8
    # offsets in front of each pair have BTYPE bits 0, and on chance pairs inside the data.)
    blocks, h = ref.Walk(r).blocks, ref.hits(r)
    pairs = {(b + 10) // 8 for b in h}
    assert [b[1] for b in blocks] == [0] * 19 and {(b[0] + 10) // 8 for b in blocks} <= pairs
    assert len(h) == 149 and len(h) <= 8 * len(pairs)


def test_walk_is_one_refs_with_the_rule_off_and_cuts_at_stored_headers_with_it_on(good):
    streams = [(w, r) for w, r, _ in good + one_ref.decoy_streams()[::3]]
    streams += [(w, r) for w, r, _ in ref.failing_streams()] + [("edge case " + c.name, c.data) for c in dc.CASES]
    fields = ("status", "err_off", "blocks", "n_units", "unit_bit", "out_off", "out_bytes", "out_len", "far", "end_bit",
              "reach")
    for what, raw in streams:
        a, b = one_ref.Walk(raw), ref.Walk(raw, stored=False)
        assert all(getattr(a, f) == getattr(b, f) for f in fields), what
        on = ref.Walk(raw)
        assert (on.status, on.err_off, on.out_len, on.out_bytes, on.blocks) == (a.status, a.err_off, a.out_len, a.out_bytes,
                                                                             a.blocks), what
        if on.status == 0:
            assert on.unit_bit[:-1] == [0] + [b[0] for b in on.blocks if b[1] in (0, 2) and b[0]], what
            assert on.out_off == [sum(b[3] for b in on.blocks if b[0] < u) for u in on.unit_bit[:-1]] + [on.out_len], what
    units = {w: (one_ref.Walk(r).n_units, ref.Walk(r).n_units) for w, r, _ in good}
    assert units["Z_FULL_FLUSH every 10 000 bytes: empty stored blocks inside units"] == (30, 60)
    assert units["text, 70 000 random bytes, text: stored blocks mid-stream"] == (3, 6)
    assert units["level 0 only: one unit"] == (1, 4)
    assert units["Z_FIXED only: one unit"] == (1, 1)


def test_hand_corpus_is_what_it_says():
    import zlib
    for what, raw, plain, units in ref.hand_streams():
        w = ref.Walk(raw)
        assert (w.status, w.n_units, w.out_bytes, w.far) == (0, units, len(plain), False), what
        assert zlib.decompress(raw, -15) == plain, what
    zero = ref.Walk(ref.hand_streams()[9][1])
    sizes = [b - a for a, b in zip(zero.out_off, zero.out_off[1:])]
    assert sizes[0] == 0 and sizes[-1] == 0 and sizes[4:7] == [0, 0, 0] and max(sizes) > 0
    inner = ref.hand_streams()[11]
    assert len(ref.candidates(inner[1])) > 2 + 6, "the inner stream's headers are candidates off the path"
    want = {"a distance one byte in front of the stream, behind a stored unit": (0, True, 2),  # (history-free: no verdict)
            "a wrong NLEN at a header the chain reaches": (ref.CORRUPT, False, 2),
            "a stored block cut short": (ref.UNEXPECTED_EOF, False, 1),
            "three bytes behind a stored header": (ref.UNEXPECTED_EOF, False, 1)}
    for what, raw, status in ref.failing_streams():
        w = ref.Walk(raw)
        assert (w.status, w.far, w.n_units) == want[what], what
        with pytest.raises(zlib.error):
            zlib.decompress(raw, -15)


def test_gzip_file_of_the_tests():
    import gzfile_ref
    members = ref.gz_members()
    f = b"".join(m for m, _ in members)
    off, on = gzfile_ref.Walk(f), ref.gzfile_walk(f)
    assert gzfile_ref.members_of(f) == [p for _, p in members]
    assert (off.status, on.status, off.n_members, on.n_members) == (0, 0, 3, 3) and off.member_off == on.member_off
    assert on.n_units > off.n_units and set(off.unit_bit) <= set(on.unit_bit)
    # the level-0 member: its first block is stored, and every block of it starts a unit
    assert on.member_unit[2] - on.member_unit[1] >= 2 and off.member_unit[2] - off.member_unit[1] == 1
    assert one_ref.Walk is not ref.Walk


def test_option_and_rule_word_checks(exe):
    out = subprocess.run([exe, "checks"], check=True, capture_output=True, text=True).stdout
    got = dict((line.split()[0], [int(v) for v in line.split()[1:]]) for line in out.splitlines())
    assert got == {
        "stored_units_0": [1], "stored_units_1": [1], "stored_units_2": [0], "stored_units_negative": [0],
        "stored_units_large": [0],
        "rule_word_at": [12, 8],
        "rule_word_0": [1, 1], "rule_word_1": [1, 1], "rule_word_2": [0, 0], "rule_word_3": [0, 0], "rule_word_4": [0, 0],
        "rule_word_alone": [1, 1],
    }
