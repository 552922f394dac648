"""The packed windows' rule and the argument checks of its three calls on the CPU: moonbit-flate_amd/csrc/seek_pack_rule.h
-- the functions the kernels and the library's host code compile -- and api_checks.h's seek_pack_args /
seek_unpack_args / one_ranges_packed_args, built with g++ into a stand-alone program under AddressSanitizer and UBSan
(arrays in allocations of exactly their size) and compared with the Python model tests/seek_pack_ref.py."""
import os
import struct
import subprocess

import pytest

import one_ref as ref
import seek_pack_ref as sp
import seek_ref as sk

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "seek_pack_rule_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(CSRC, "seek_pack_rule.h"), os.path.join(CSRC, "seek_index_rule.h"),
        os.path.join(CSRC, "bgzf_range_rule.h"), os.path.join(CSRC, "bgzf_rule.h"), os.path.join(CSRC, "api_checks.h"),
        os.path.join(INC, "flate_hip.h")]
EXE = os.path.join(HERE, "host_model", "seek_pack_rule_model")
INVALID = -1
W = sp.WINDOW


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + INC, SRC, "-o", EXE])
    return EXE


def keep_grid():
    """(q, len, dist, P0) around every edge of the rule: q = P0 and q = P0 + 32767 / + 32768, dist = 32768, 32767, 1, 2,
    3, len 3 and 258, copies that straddle P0, P0 < 32768 -- and what lies one step outside the rule's domain."""
    cases = []
    for P0 in (0, 1, 5, 258, 32767, 32768, 32769, 100000, (1 << 40) + 7):
        for dq in (0, 1, 2, 3, 255, 257, 258, 259, 32509, 32510, 32511, 32765, 32766, 32767, 32768, 32769):
            for dist in (1, 2, 3, 4, 257, 258, 259, 260, 32510, 32766, 32767, 32768):
                for ln in (3, 4, 258):
                    cases.append((P0 + dq, ln, dist, P0))
        cases += [(P0 - 1 if P0 else 0, 3, 1, P0), (P0, 0, 1, P0), (P0, 3, 0, P0), (P0, 3, 32769, P0), (P0, 258, 0xffffffff, P0)]
    return cases


def test_the_grid_holds_every_kind_of_answer():
    got = [sp.keep(*c) for c in keep_grid()]
    assert (0, 0) in got and (0, 3) in got and (W - 1, W) in got and (W - 258, W) in got
    assert any(hi - lo == 258 and hi < W for lo, hi in got)        # a copy wholly in front of P0
    assert any(0 < hi - lo < 3 and hi == W for lo, hi in got)      # a copy that straddles P0: clipped at P0
    assert any(lo == W - 5 and hi == W for lo, hi in got)          # P0 = 5: clipped at the stream's first byte
    # an overlapping copy (dist < len) that starts in front of P0 keeps only its source bytes in front of P0
    assert sp.keep(100000, 258, 2, 100000) == (W - 2, W) and sp.keep(100001, 258, 3, 100000) == (W - 2, W)
    assert sp.keep(100000 + 32767, 3, 32768, 100000) == (W - 1, W) and sp.keep(100000 + 32768, 3, 32768, 100000) == (0, 0)


def test_seek_pack_keep_equals_the_python_interval(exe, tmp_path):
    cases = keep_grid()
    blob = struct.pack("<I", len(cases)) + b"".join(struct.pack("<QIIQ", *c) for c in cases)
    path = tmp_path / "keep.bin"
    path.write_bytes(blob)
    lines = subprocess.run([exe, "keep", str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(cases) > 5000
    for c, line in zip(cases, lines):
        assert tuple(int(x) for x in line.split()) == sp.keep(*c), c


@pytest.fixture(scope="module")
def packed_index():
    """(the seek index's words, a pack index for it with an empty block among full ones, packed_bytes)."""
    what, raw, plain = ref.good_streams()[ref.MANY_UNITS]
    w = ref.Walk(raw)
    index = sk.index_words(w, plain, len(raw), ref.GZIP, 40000)
    nb = index[9] - 1
    sizes = [700 + 13 * b for b in range(nb)]
    sizes[0] = sizes[3] = 0
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return index, sp.pack_words(index, sp.COMPRESS | sp.SPARSE, off, 12345), off[-1]


def test_seek_pack_ok_refuses_one_violation_of_every_clause(exe, packed_index, tmp_path):
    index, words, pb = packed_index
    other = list(index)
    other[9] += 1  # (only the head is read)
    cases = [("sound", words, pb, index, True), ("sound, COMPRESS alone", sp.pack_words(index, sp.COMPRESS, words[16:], (index[9] - 1) * W),
                                                 pb, index, True)]
    cases += [(what, wd, b, index, False) for what, wd, b in sp.violations(words, pb)]
    cases.append(("COMPRESS alone with fewer kept bytes than the whole", sp.pack_words(index, sp.COMPRESS, words[16:], 5), pb, index, False))
    cases.append(("an index with one point more", words, pb, other, False))
    cases.append(("fewer words than the head and off[0]", words[:16], pb, index, False))
    cases.append(("no words", [], pb, index, False))
    blob = struct.pack("<I", len(cases))
    for _, wd, b, ix, _ in cases:
        blob += struct.pack("<QQ", b, len(wd)) + struct.pack("<%dQ" % len(wd), *[x & sk.U64 for x in wd])
        blob += struct.pack("<Q", len(ix)) + struct.pack("<%dQ" % len(ix), *ix)
    path = tmp_path / "pack.bin"
    path.write_bytes(blob)
    lines = subprocess.run([exe, "ok", str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(cases)
    binding = ("is not the index's", "one point more", "one block more")
    for (what, wd, b, ix, want), line in zip(cases, lines):
        ok, self_ok = (int(x) for x in line.split())
        assert sp.pack_ok(wd, b, ix) == want, what  # the Python model agrees with the hand-made verdict ...
        assert (ok == 1) == want, what               # ... and so does the header
        if not want and not any(k in what for k in binding):
            assert self_ok == 0, what                # (what unpack sees: everything but the binding)


def test_seek_pack_head_equals_the_python_words(exe, packed_index, tmp_path):
    index, words, pb = packed_index
    path = tmp_path / "head.bin"
    path.write_bytes(struct.pack("<IQQQ", 3, pb, 12345, len(index)) + struct.pack("<%dQ" % len(index), *index))
    out = subprocess.run([exe, "head", str(path)], check=True, capture_output=True, text=True).stdout
    assert [int(x) for x in out.split()] == words[:16]


def test_argument_checks(exe):
    out = subprocess.run([exe, "checks"], check=True, capture_output=True, text=True).stdout
    got = dict((k, int(v)) for k, v in (line.split() for line in out.splitlines()))
    assert got == {
        "pack_ok": 0, "pack_no_in_compress": 0, "pack_query": 0,
        "pack_no_in_sparse": INVALID, "pack_mode_0": INVALID, "pack_mode_sparse_alone": INVALID, "pack_mode_4": INVALID,
        "pack_flag_go": INVALID, "pack_wrap_3": INVALID, "pack_wrap_not_the_index": INVALID, "pack_no_pack_words": INVALID,
        "pack_no_packed_bytes": INVALID, "pack_no_kept_bytes": INVALID, "pack_no_pack_index_with_cap": INVALID,
        "pack_no_packed_with_cap": INVALID, "pack_windows_without_buffer": INVALID, "pack_no_index": INVALID,
        "unpack_ok": 0, "unpack_no_windows_bytes": INVALID, "unpack_no_pack_index": INVALID,
        "unpack_short_pack_index": INVALID, "unpack_no_windows_with_cap": INVALID, "unpack_flag_size_only": INVALID,
        "read_ok": 0, "read_size_query": 0, "read_no_index": INVALID, "read_no_pack_index": INVALID,
        "read_backwards": INVALID, "read_wrap_not_the_index": INVALID, "read_packed_without_buffer": INVALID,
        "read_pack_of_another_index": INVALID,
    }
