"""The rule of ONE stream read in parts on the CPU: moonbit-flate_amd/csrc/one_parts_rule.h -- the functions the part
kernels and flate_hip_one_reader_read compile -- and api_checks.h's one_reader_*_args, built with g++ into a stand-alone
program under AddressSanitizer and UBSan and compared with the Python reference tests/one_parts_ref.py: the header's
three answers at every cut of a gzip header with FEXTRA, FNAME, FCOMMENT and FHCRC, and whole readers -- every call's
status, in_used, out_len, n_units and err_off -- at every cut position of a few short streams, with small capacities,
with the trailer cut at each of its positions, with wrong trailers, truncated and corrupt streams and junk behind the
trailer.  The reference itself is held against zlib: the bytes, the end of the stream and the sum of in_used."""
import os
import struct
import subprocess
import zlib

import pytest

import gzip_ref
import one_parts_ref as R
import one_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "one_parts_rule_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(INC, "flate_hip.h")] + [os.path.join(CSRC, h) for h in ("one_parts_rule.h", "api_checks.h", "gzip_rule.h")]
EXE = os.path.join(HERE, "host_model", "one_parts_rule_model")
KINDS = (R.RAW, R.ZLIB, R.GZIP)


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


@pytest.fixture(scope="module")
def streams():
    """[(what, raw, plain)]: short streams of several units each, computed once, shared, never changed."""
    t = gzip_ref.text(6000, seed=33)
    mixed = t[:2500] + gzip_ref.rand(700, seed=4) + t[2500:]
    out = [("level 6, memLevel 1", ref.deflate(t, 6, mem=1), t),
           ("level 1, memLevel 1", ref.deflate(t[:4000], 1, mem=1), t[:4000]),
           ("text, random bytes, text: stored blocks", ref.deflate(mixed, 6, mem=1), mixed),
           ("Z_FULL_FLUSH every 900 bytes", ref.deflate(t[:4000], 6, mem=1, flush_every=900), t[:4000])]
    for what, raw, plain in out:
        w = ref.Walk(raw)
        assert w.status == 0 and w.n_units >= 8 and zlib.decompress(raw, -15) == plain, what
    return out


# ---- a recorded reader: the reference decides, the rule is asked the same questions ----

class Recorded:
    def __init__(self, f, kind, unit_max=1 << 28):
        self.m = R.Model(f, kind, unit_max)
        self.lines, self.expect = ["N %d %d" % (kind, unit_max)], []
        self.model_read = R.model_reader(self.m)

    def read(self, buf, final, out_cap):
        m = self.m
        cap = out_cap if out_cap is not None else 1 << 62
        rc, err, fu, fo, ok, bits, offs = 99, -1, 0, 0, 1, [0], [0]
        if m.status == 0 and m.pending:
            ok = int(m._trailer_ok(m.consumed))
        elif m.status == 0 and len(buf):
            d = m.discovery(len(buf), final)
            if d.hdr == R.GOOD and d.rc is not None:
                rc, err, fu, fo, bits, offs = d.rc, d.err_off, d.fail_unit, d.fail_out, d.unit_bit, d.out_off
                if d.rc == 0:
                    ok = int(m._trailer_ok(m.consumed + d.raw_off + (bits[-1] + 7) // 8))
        self.lines.append("R %d %d %d %s %d %d %d %d %d %d %s %s" % (
            len(buf), final, cap, "-" if m.header_done else hexs(buf[:64]), rc, err, fu, fo, ok, len(bits) - 1,
            " ".join(map(str, bits)), " ".join(map(str, offs))))
        c, got = self.model_read(buf, final, out_cap)
        self.expect.append(c)
        return c, got

    def check(self, exe, tmp_path, what):
        got = run(exe, self.lines, tmp_path)
        want = ["%d %d %d %d %d" % c for c in self.expect]
        assert got == want, (what, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:3])


def whole_and_true(rec, f, plain, sizes, out_cap, units, what, grow=1):
    """Feed f in parts; the reference must deliver zlib's bytes, end the stream and use every byte of the member."""
    calls, out, rest = R.feed(rec.read, f, sizes, out_cap, units + len(f) + 8, grow)  # (at most len(f) parts)
    assert calls[-1].rc == R.STREAM_END and out == plain and not rest, (what, calls[-1])
    assert sum(c.in_used for c in calls) == len(f) and sum(c.n_units for c in calls) == units, what
    return calls


# ---- the header's three answers ----

def gzip_header(extra=b"", name=None, comment=None, hcrc=False):
    flg = (4 if extra else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    h = bytes([0x1f, 0x8b, 8, flg, 1, 2, 3, 4, 0, 3])
    if extra:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xffff)
    return h


def test_a_header_cut_at_every_byte(exe, tmp_path, streams):
    _, raw, plain = streams[0]
    headers = [(R.GZIP, gzip_header(b"ab\x05\x00hello", b"a name.txt", b"and a comment", True)),
               (R.GZIP, gzip_header(b"\0\0\0\0", b"")), (R.GZIP, gzip_header()), (R.GZIP, gzip_header(name=b"n")),
               (R.ZLIB, b"\x78\x9c"), (R.ZLIB, b"\x78\x01")]
    lines, want = [], []
    for kind, h in headers:
        tail = raw + (struct.pack("<II", zlib.crc32(plain), len(plain)) if kind == R.GZIP else
                      struct.pack(">I", zlib.adler32(plain)))
        # the truth: zlib reads the member, and the raw stream starts right behind the header
        assert zlib.decompress(h + tail, 31 if kind == R.GZIP else 15) == plain
        assert R.header_state(kind, h + tail) == (R.GOOD, len(h))
        for cut in range(len(h) + 3):
            st = R.header_state(kind, (h + tail)[:cut])
            assert st == ((R.GOOD, len(h)) if cut >= len(h) else (R.MORE, 0)), (kind, cut)
            lines.append("H %d %s" % (kind, hexs((h + tail)[:cut])))
            want.append("%d %d" % st)
            for final in (0, 1):  # a final part: what is refused for want of bytes is bad; the trailer must fit
                lines.append("F %d 1 %d %s" % (kind, final, hexs((h + tail)[:cut])))
                tl = R.TRAILER[kind]
                bad = final and (cut < len(h) + tl)
                hdr = R.BAD if bad else st[0]
                want.append("%d %d %d" % (hdr, len(h) if hdr == R.GOOD else 0,
                                          (cut - tl if final else cut) if hdr == R.GOOD else 0))
        for at in range(len(h)):  # one wrong bit anywhere in the bytes the rule judges
            bad = bytearray(h + tail)
            bad[at] ^= 0x80 if (kind == R.GZIP and at == 3) or kind == R.ZLIB else 0x01
            st = R.header_state(kind, bad[:max(at + 1, 2 if kind == R.ZLIB else 1)])
            lines.append("H %d %s" % (kind, hexs(bad[:max(at + 1, 2 if kind == R.ZLIB else 1)])))
            want.append("%d %d" % st)
            if kind == R.ZLIB or at < 4:
                assert st[0] == R.BAD, (kind, at)
    # zlib with a preset dictionary: bad (no dictionaries here); later parts and raw streams have no header
    fdict = bytes([0x78, 0x20 | (31 - (0x7820 % 31))])
    assert (fdict[0] * 256 + fdict[1]) % 31 == 0 and R.header_state(R.ZLIB, fdict) == (R.BAD, 0)
    lines += ["H 1 " + hexs(fdict), "H 0 -", "F 2 0 0 0102030405", "F 2 0 1 010203040506070809", "F 2 0 1 0102", "F 0 1 1 01"]
    want += ["1 0", "0 0", "0 0 5", "0 0 1", "0 0 0", "0 0 1"]
    assert run(exe, lines, tmp_path) == want


# ---- whole readers ----

def test_every_cut_position_of_short_streams(exe, tmp_path, streams):
    t = gzip_ref.text(4000, seed=34)
    b0 = set()
    for what, raw, plain in (("4000 bytes, level 6", ref.deflate(t, 6, mem=1), t), ("level 1", ref.deflate(t, 1, mem=1), t)):
        units = ref.Walk(raw).n_units
        assert units >= 8
        for kind in KINDS:
            f = ref.wrap(raw, plain, kind)
            rec = Recorded(f, kind)
            for cut in range(len(f) + 1):
                rec.m.reset()
                rec.lines.append("N %d %d" % (kind, 1 << 28))
                calls = whole_and_true(rec, f, plain, [cut], None, units, (what, kind, cut))
                b0.add(rec.m.w.unit_bit[calls[0].n_units] % 8 if calls[0].n_units else None)
            rec.check(exe, tmp_path, (what, kind))
    assert b0 >= set(range(8)), b0  # every carry bit occurs where a first call stops


def test_small_parts_small_capacities_and_growing_parts(exe, tmp_path, streams):
    for what, raw, plain in streams:
        w = ref.Walk(raw)
        biggest = max(b - a for a, b in zip(w.out_off, w.out_off[1:]))
        for kind in KINDS:
            f = ref.wrap(raw, plain, kind)
            rec = Recorded(f, kind)
            for step, cap in ((1, None), (7, None), (64, biggest), (300, biggest + 50), (len(f), biggest), (97, 1 << 20)):
                rec.m.reset()
                rec.lines.append("N %d %d" % (kind, 1 << 28))
                whole_and_true(rec, f, plain, iter(lambda: step, 0), cap, w.n_units, (what, kind, step, cap))
            rec.check(exe, tmp_path, (what, kind))


def test_a_first_unit_that_does_not_fit_changes_nothing(exe, tmp_path, streams):
    what, raw, plain = streams[0]
    w = ref.Walk(raw)
    f = ref.wrap(raw, plain, R.GZIP)
    rec = Recorded(f, R.GZIP)
    first = w.out_off[1]
    c, _ = rec.read(f[:900], False, first - 1)
    assert c == R.Call(R.OUT_TOO_SMALL, 0, first, 0, -1)
    c, got = rec.read(f[:900], False, first)
    assert (c.rc, c.out_len, c.n_units) == (R.OK, first, 1) and got == plain[:first]
    rest = f[c.in_used:]
    c2, _ = rec.read(rest, True, 0)  # not even the next unit: its size is asked for, the state stays
    assert c2 == R.Call(R.OUT_TOO_SMALL, 0, w.out_off[2] - first, 0, -1)
    c3, got = rec.read(rest, True, 1 << 20)
    assert c3.rc == R.STREAM_END and got == plain[first:]
    # a part of at least one_unit_max bytes that completes no unit
    big = Recorded(f, R.GZIP, unit_max=40)
    c, _ = big.read(f[:39], False, 1 << 20)
    assert c == R.Call(R.OK, 0, 0, 0, -1)
    c, _ = big.read(f[:40], False, 1 << 20)
    assert c.rc == R.TOO_LARGE
    assert big.read(f[:500], False, 1 << 20)[0].rc == R.TOO_LARGE  # sticky
    rec.check(exe, tmp_path, what)
    big.check(exe, tmp_path, what)


def test_the_trailer_cut_at_each_position_wrong_trailers_and_junk(exe, tmp_path, streams):
    what, raw, plain = streams[0]
    units = ref.Walk(raw).n_units
    for kind in (R.ZLIB, R.GZIP):
        f = ref.wrap(raw, plain, kind)
        tl = R.TRAILER[kind]
        rec = Recorded(f, kind)
        for j in range(tl + 1):  # the first part holds the final block and j bytes of the trailer
            rec.m.reset()
            rec.lines.append("N %d %d" % (kind, 1 << 28))
            calls = whole_and_true(rec, f, plain, [len(f) - tl + j], None, units, (kind, j), grow=1)
            if j < tl:
                assert (calls[0].rc, calls[0].in_used, calls[0].out_len) == (R.OK, len(f) - tl, len(plain)), (kind, j)
                assert calls[-1] == R.Call(R.STREAM_END, tl, 0, 0, -1), (kind, j)
            else:
                assert len(calls) == 1
        rec.check(exe, tmp_path, (what, kind))
        # a truncated trailer on a final part: the end of input
        rec = Recorded(f[:-1], kind)
        calls, out, _ = R.feed(rec.read, f[:-1], [len(f) - tl], None, 8)
        assert [c.rc for c in calls] == [R.OK, R.EOF] and out == plain
        assert rec.read(b"", True, 0)[0].rc == R.EOF  # sticky
        rec.check(exe, tmp_path, (what, kind, "short trailer"))
        # a wrong checksum / length: the last call fails, err_off = the member's length
        for at in ((-1, -5) if kind == R.GZIP else (-1,)):
            g = bytearray(f)
            g[at] ^= 0x10
            for sizes in ([len(f)], [len(f) - tl], [len(f) // 2]):
                rec = Recorded(bytes(g), kind)
                calls, out, _ = R.feed(rec.read, bytes(g), sizes, None, units + 8)
                assert (calls[-1].rc, calls[-1].err_off) == (R.CORRUPT, len(f)) and out == plain, (kind, at, sizes)
                assert rec.read(b"x", False, 9)[0] == R.Call(R.CORRUPT, 0, 0, 0, len(f))
                rec.check(exe, tmp_path, (what, kind, at))
        # junk behind the trailer is left unused
        g = f + b"junk behind the member"
        for sizes in ([len(g)], [len(f) - 3], [1000]):
            rec = Recorded(g, kind)
            calls, out, rest = R.feed(rec.read, g, sizes, None, units + 8)
            assert calls[-1].rc == R.STREAM_END and out == plain and sum(c.in_used for c in calls) == len(f), (kind, sizes)
            assert g.endswith(rest) and rest.startswith(b"junk"[:len(rest)]) or not rest
            rec.check(exe, tmp_path, (what, kind, "junk"))


def test_truncated_and_corrupt_streams(exe, tmp_path, streams):
    what, raw, plain = streams[0]
    w = ref.Walk(raw)
    for kind in KINDS:
        f = ref.wrap(raw, plain, kind)
        for end in (len(f) // 2, len(f) - R.TRAILER[kind] - 1):
            g = f[:end]
            for sizes in ([len(g)], [len(g) // 3], iter(lambda: 200, 0)):
                rec = Recorded(g, kind)
                calls, out, _ = R.feed(rec.read, g, sizes, None, w.n_units + len(g) // 200 + 8, grow=200)
                assert calls[-1].rc == R.EOF and plain.startswith(out), (kind, end)
                # what the serial decoder delivers of the stream whose last bytes are taken for the trailer
                cut = ref.Walk(g[ref.header_len(kind):len(g) - R.TRAILER[kind]]).out_len
                assert len(out) == cut if len(calls) == 1 else len(out) >= cut, (kind, end)
                rec.check(exe, tmp_path, (what, kind, end))
    # a reserved block type in the middle of the stream: the stream's verdict at the serial offset, the bytes in front
    k = next(k for k in range(w.n_units // 2, w.n_units) if w.unit_bit[k] % 8 < 6)  # (both type bits in one byte)
    bit = w.unit_bit[k]
    g = bytearray(raw)
    g[bit // 8] |= 3 << (bit % 8 + 1)  # BTYPE = 3 in the header that starts unit k: unit k - 1 runs into it
    wb = ref.Walk(bytes(g))
    assert wb.status == R.CORRUPT and wb.n_units == k - 1 and wb.out_len == w.out_off[k]
    for sizes in ([len(g)], [len(g) // 3], iter(lambda: 100, 0)):
        rec = Recorded(bytes(g), R.RAW)
        calls, out, _ = R.feed(rec.read, bytes(g), sizes, None, w.n_units + len(g) // 100 + 8, grow=100)
        assert (calls[-1].rc, calls[-1].err_off) == (R.CORRUPT, wb.err_off) and out == plain[:wb.out_len], sizes
        rec.check(exe, tmp_path, (what, "corrupt", sizes))


def test_argument_checks(exe):
    got = dict(l.split() for l in subprocess.check_output([exe, "checks"]).decode().split("\n") if l)
    ok = {k for k, v in got.items() if v == "0"}
    assert ok == {"open_ok", "open_raw_ok", "read_ok", "read_nothing_ok"}
    assert all(v == "-1" for k, v in got.items() if k not in ok) and len(got) == 13
