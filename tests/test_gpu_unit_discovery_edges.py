"""The branches in which the two-list discoveries differ (csrc/unit_discovery.h and its users in flate_api_units.hip),
each with a few KiB of input, every expectation from zlib on the CPU:

  * a gzip file with nothing for FIND: every member's payload is one final STORED block of zeros, so List A holds bit 0
    alone (always a candidate, never on the path) and every unit comes from List B;
  * a part that lies wholly inside one member: List B of that part is empty;
  * a part that ends inside a gzip header: the root cannot be judged, first with more to come, then as the file's end;
  * a ZIP entry through units whose hull has no candidate behind bit 0 (one B node);
  * "gzfile_serial_max" with every member whole: the bit search is skipped (find_from == the file's length);
  * the same file with one long last member: the search runs over that member alone.
"""
import random
import struct
import zlib

import numpy as np
import pytest

from util import flate

pytestmark = pytest.mark.gpu

GZ_HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"
NAMED_HEADER = b"\x1f\x8b\x08\x08\x00\x00\x00\x00\x00\xff" + b"a-name-of-some-length.txt\x00"
CORRUPT, EOF, STREAM_END = -4, -7, 1
CHUNK = 12000  # bytes of text per unit: one dynamic block at level 6


def text(n, seed):
    rnd = random.Random(seed)
    words = ["".join(chr(rnd.randrange(97, 123)) for _ in range(rnd.randrange(2, 9))) for _ in range(400)]
    out = " ".join(rnd.choice(words) for _ in range(n // 3)).encode()
    assert len(out) >= n
    return out[:n]


def flushed(chunks):
    """One raw stream, a full flush behind every chunk but the last: every chunk is one dynamic block and one unit."""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return b"".join(c.compress(p) + c.flush(zlib.Z_FULL_FLUSH) for p in chunks[:-1]) + c.compress(chunks[-1]) + c.flush()


def stored_final(plain):
    assert len(plain) < 65536
    return b"\x01" + struct.pack("<HH", len(plain), len(plain) ^ 0xFFFF) + plain


def member(plain, raw, header=GZ_HEADER):
    assert zlib.decompress(raw, -15) == plain
    return header + raw + struct.pack("<II", zlib.crc32(plain), len(plain))


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def chunks():
    return [text(CHUNK, 300 + k) for k in range(4)]


@pytest.fixture(scope="module")
def short_members():
    plains = [text(700 + 90 * k, 40 + k) for k in range(3)]
    return b"".join(member(p, zlib.compress(p, 6)[2:-4]) for p in plains), b"".join(plains)


def feed(rd, f, ends, out_cap=None):
    """The file through a reader, a part per entry of `ends` (every part begins with what the last call left unused);
    -> ([(rc, in_used, n_members, n_units)], the bytes).  The loop ends with the file's end or its error."""
    calls, got, pos = [], b"", 0
    for end in ends:
        for _ in range(8):  # (a call that delivers less than it found is made again over the rest)
            used, out, r = rd.read(f[pos:end], final=end == len(f), out_cap=out_cap)
            calls.append((r.rc, used, getattr(r, "n_members", None), r.n_units))
            got += bytes(out)
            pos += used
            if r.rc != 0 or used == 0 or pos == end:
                break
        if calls[-1][0] != 0:
            break
    return calls, got


def test_gzfile_of_final_stored_blocks(eng):
    plains = [bytes(n) for n in (1, 700, 3000)]
    f = b"".join(member(p, stored_final(p)) for p in plains)
    plain = b"".join(plains)
    ix = eng.gzfile_index(f)
    assert (ix.rc, ix.status, ix.n_members, ix.n_units, ix.out_bytes) == (0, 0, 3, 3, len(plain))
    for data in (f, np.frombuffer(f, np.uint8)):
        out, r = eng.gzfile_read(data)
        assert (r.rc, r.n_members, r.n_units) == (0, 3, 3) and bytes(out[:r.out_len]) == plain
    rd = eng.open_gzfile_reader()
    try:
        calls, got = feed(rd, f, [len(GZ_HEADER) + 3, len(f) - 5, len(f)])
        assert calls[-1][0] == STREAM_END and got == plain and sum(c[2] for c in calls) == 3
    finally:
        rd.close()


def test_a_part_wholly_inside_one_member(eng, chunks):
    raw = flushed(chunks)
    plain = b"".join(chunks)
    f = member(plain, raw)
    third = len(f) // 3
    assert GZ_HEADER not in f[third:2 * third]  # no header, not even a false one, in the middle part
    rd = eng.open_gzfile_reader()
    try:
        calls, got = feed(rd, f, [third, 2 * third, len(f)])
        assert calls[-1][0] == STREAM_END and got == plain
        assert sum(c[2] for c in calls) == 1 and sum(c[3] for c in calls) == len(chunks)
        assert any(c[0] == 0 and c[3] >= 1 and c[2] == 0 for c in calls[1:]), calls  # units delivered from inside
    finally:
        rd.close()


def test_a_part_that_ends_inside_a_gzip_header(eng, short_members):
    p0, p1 = text(900, 7), text(1100, 8)
    m0, m1 = member(p0, zlib.compress(p0, 6)[2:-4]), member(p1, zlib.compress(p1, 6)[2:-4], NAMED_HEADER)
    f = m0 + m1
    for inside in (3, 12, len(NAMED_HEADER) - 1):  # the fixed part, the name, one byte short
        cut = len(m0) + inside
        rd = eng.open_gzfile_reader()
        try:
            # not final: the first member is delivered, the cut header waits; then the rest
            calls, got = feed(rd, f, [cut, len(f)])
            assert calls[0][:3] == (0, len(m0), 1) and calls[-1][0] == STREAM_END and got == p0 + p1, (inside, calls)
            # a part that is nothing but the cut header: more is needed, nothing moves
            rd.reset()
            used, out, r = rd.read(f[:len(m0)], final=False)
            assert (r.rc, used, bytes(out)) == (0, len(m0), p0)
            used, out, r = rd.read(m1[:inside], final=False)
            assert (r.rc, used, r.out_len) == (0, 0, 0)
            # final: the file ends inside the header
            used, out, r = rd.read(m1[:inside], final=True)
            assert (r.rc, used, r.out_len, r.bad_member, r.err_off) == (CORRUPT, 0, 0, 1, len(m0)), inside
        finally:
            rd.close()


def archive(raw, plain):
    name = b"e0"
    crc = zlib.crc32(plain)
    local = struct.pack("<4sHHHHHIIIHH", b"PK\3\4", 20, 0x0800, 8, 0, 0x0021, crc, len(raw), len(plain), len(name), 0) + name
    central = struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\1\2", 20, 20, 0x0800, 8, 0, 0x0021, crc, len(raw), len(plain),
                          len(name), 0, 0, 0, 0, 0, 0) + name
    return local + raw + central + struct.pack("<4sHHHHIIH", b"PK\5\6", 0, 0, 1, 1, len(central), len(local) + len(raw), 0)


def test_zip_units_over_a_hull_without_candidates(eng):
    plain = bytes(2500)
    eng.set_option("zip_unit_min", 1)
    try:
        out, r = eng.zip_read(archive(stored_final(plain), plain))
        route = eng.zip_last_route()
    finally:
        eng.set_option("zip_unit_min", 0)
    assert r.rc == 0 and int(r.out_len[0]) == len(plain) and bytes(out[:len(plain)]) == plain
    assert route[:3] == (1, 0, 1), route  # served by units: one entry, one unit


def test_serial_max_with_every_member_whole(eng, short_members, chunks):
    f, plain = short_members
    long_plain = b"".join(chunks)
    with_long = f + member(long_plain, flushed(chunks))
    eng.set_option("gzfile_serial_max", 4096)
    try:
        out, r = eng.gzfile_read(f)
        assert (r.rc, r.n_members, r.n_units) == (0, 3, 3) and bytes(out[:r.out_len]) == plain
        assert eng.gzfile_last_route() == (3, 0, len(f))  # phase 2 skipped: nothing to search
        ix = eng.gzfile_index(f)
        assert (ix.rc, ix.n_members, ix.n_units, ix.out_bytes) == (0, 3, 3, len(plain))
        assert eng.gzfile_last_route() == (3, 0, len(f))
        # ... plus one long last member: the search runs from that member on
        out, r = eng.gzfile_read(with_long)
        assert (r.rc, r.n_members, r.n_units) == (0, 4, 3 + len(chunks)) and bytes(out[:r.out_len]) == plain + long_plain
        assert eng.gzfile_last_route() == (3, 1, len(f))
    finally:
        eng.set_option("gzfile_serial_max", 0)
