"""The tile geometry of the byte-offset discoveries (flate_hip_bgzf_index, flate_hip_gzip_index, flate_hip_zip_index):
one workgroup tests every offset of a 4 KiB tile (plus 16 bytes of halo) on the grid of the buffer's ADDRESS
(chain_walk.h: tile_load and the tile pass, which all three share with flate_hip_inflate_one_index, whose own placed
headers are tests/test_gpu_inflate_one_tiles.py).  Here a header is PLACED: padding in the first member -- the stored
payload of a BGZF member, the FNAME of a gzip member, the name of a ZIP archive's first central record -- moves the
SECOND header to every byte from 17 in front of a tile boundary to 1 behind it, the device tensor's shift moves the
buffer to the alignments 0, 1 and 15; once the placed header is the chain's second member, once it is a decoy that
no chain reaches.  Every expectation is the serial reference's (bgzf_ref.Walk, gzip_ref.Walk, zip_ref.Index) on the
same bytes."""
import zlib

import pytest

import bgzf_ref
import gzip_ref
import zip_ref
import test_gpu_bgzf as tb
import test_gpu_gzip as tg
import test_gpu_zip as tz
from util import flate

gpu = pytest.mark.gpu  # (the one test without it checks the placed files themselves, on the CPU)

TILE = 4096  # kTileBytes
OFFSETS = tuple(range(-17, 2))  # the header's first byte against the tile boundary: the last bytes of a tile read the halo
ALIGNS = (0, 1, 15)
SECOND = gzip_ref.text(300, seed=4)
FILL = bytes(range(1, 30)) * 300  # (padding without a NUL, a gzip magic or a ZIP signature)


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


def boundary(delta):
    """The tile boundary the header is placed at: both inner ones of a file of three tiles."""
    return TILE * (1 + delta % 2)


# ---- the placed files: (file, what it inflates to, the placed header's offset) ----

def bgzf_file(v, A, decoy):
    at = v - A
    if decoy:  # a complete header that claims 26 bytes, inside the first member's stored payload
        pay = bytearray(FILL[:at - 23 + 40])
        pay[at - 23:at - 23 + 18] = bgzf_ref.decoy_header(26)
        pay = bytes(pay)
    else:  # the first member has exactly `at` bytes
        pay = FILL[:at - 31]
    f = bgzf_ref.stored_member(pay) + bgzf_ref.zlib_member(SECOND) + bgzf_ref.EOF
    return f, pay + SECOND, at


def gzip_file(v, A, decoy):
    at = v - A
    if decoy:  # a header with an empty stored stream and a trailer, at the start of the first member's stored payload
        name = FILL[:at - 10 - 1 - 5]
        pay = gzip_ref.header() + b"\x01\x00\x00\xff\xff" + bytes(8) + b"behind the decoy"
        first = gzip_ref.stored(pay, flg=gzip_ref.FNAME, name=name)
    else:
        pay = b"first"
        head = len(gzip_ref.stored(pay, flg=gzip_ref.FNAME, name=b""))
        first = gzip_ref.stored(pay, flg=gzip_ref.FNAME, name=FILL[:at - head])
    return first + gzip_ref.member(SECOND), pay + SECOND, at


def zip_file(v, A, decoy):
    datas = [b"first entry", SECOND, b"third"]
    raws = [gzip_ref.raw(d) for d in datas]
    rec = zip_ref.central_record(b"d", 0, 0, 0, 0)  # a well-formed central record: inside a name it is a decoy
    # the first name's length moves the second record, and every name moves cd_off: the two lengths that fit
    for pad in range(v - 46 - 15, v - 46 + 1):
        for more in range(16):
            names = [FILL[:pad] + (rec if decoy else b""), b"second" + b"x" * more, b"3"]
            f, entry_off = zip_ref.write_archive(raws, names, [zlib.crc32(d) for d in datas], [len(d) for d in datas])
            cd_off = entry_off[-1]
            at = cd_off + 46 + pad
            if at + A - ((cd_off + A) & ~15) == v:  # (ZIP's tiles count from (cd_off + A) & ~15)
                return f, b"".join(datas), at
    raise AssertionError("no name length places the record")


CASES = [(fmt, A, delta, decoy) for fmt in ("bgzf", "gzip", "zip") for A in ALIGNS for delta in OFFSETS for decoy in (False, True)]
MAKE = {"bgzf": bgzf_file, "gzip": gzip_file, "zip": zip_file}


def test_the_placed_files_are_what_they_claim():
    """On the CPU: the serial references accept every file, the placed header is where it should be and passes the
    format's rule there, and it is the chain's second member -- or, as a decoy, on no chain."""
    for fmt, A, delta, decoy in CASES:
        v = boundary(delta) + delta
        f, plain, at = MAKE[fmt](v, A, decoy)
        what = (fmt, A, delta, decoy)
        assert fmt == "zip" or len(f) + A <= 3 * TILE, what  # (ZIP: the directory's tiles, below)
        if fmt == "bgzf":
            w = bgzf_ref.Walk(f)
            assert (w.rc, w.n_members) == (0, 3) and (w.member_off[1] == at) == (not decoy), what
            assert bgzf_ref.member_total(f, at) == (26 if decoy else w.member_off[2] - at) and at + A == v, what
        elif fmt == "gzip":
            w = gzip_ref.Walk(f)
            assert (w.rc, w.n_members, w.n_candidates) == (0, 2, 3 if decoy else 2), what
            assert (w.member_off[1] == at) == (not decoy) and at in [c[0] for c in w.table] and at + A == v, what
            assert gzip_ref.plain_of(f) == plain, what
        else:
            ix = zip_ref.Index(f)
            cd_off, cd_end = ix.end.cd_off, ix.end.cd_off + ix.end.cd_size
            assert (ix.rc, ix.n_entries) == (0, 3) and (cd_end - cd_off + 15) // TILE + 1 <= 3, what
            assert zip_ref.central_read(f, at, cd_end) is not None, what
            assert (ix.entries[1].name_off - 46 == at) == (not decoy), what


@gpu
@pytest.mark.parametrize("A", ALIGNS)
@pytest.mark.parametrize("decoy", (False, True), ids=("member", "decoy"))
def test_bgzf_header_at_every_byte_around_a_tile_boundary(eng, A, decoy):
    for delta in OFFSETS:
        f, plain, _ = bgzf_file(boundary(delta) + delta, A, decoy)
        what = "bgzf header at %+d, A = %d, decoy %d" % (delta, A, decoy)
        tb.check_index(eng, f, what, device=True, shift=A)
        tb.check_read_good(eng, f, plain, what, device=True, shift=A, out_shift=1)


@gpu
@pytest.mark.parametrize("A", ALIGNS)
@pytest.mark.parametrize("decoy", (False, True), ids=("member", "decoy"))
def test_gzip_header_at_every_byte_around_a_tile_boundary(eng, A, decoy):
    for delta in OFFSETS:
        f, plain, _ = gzip_file(boundary(delta) + delta, A, decoy)
        w = gzip_ref.Walk(f)
        what = "gzip header at %+d, A = %d, decoy %d" % (delta, A, decoy)
        assert tg.check_index(eng, f, w, what, device=True, shift=A) == (3 if decoy else 2), what  # (n_candidates)
        tg.check_read_good(eng, f, plain, w, what, device=True, shift=A, out_shift=1)


@gpu
@pytest.mark.parametrize("A", ALIGNS)
@pytest.mark.parametrize("decoy", (False, True), ids=("record", "decoy"))
def test_zip_record_at_every_byte_around_a_tile_boundary(eng, A, decoy):
    for delta in OFFSETS:
        f, plain, _ = zip_file(boundary(delta) + delta, A, decoy)
        what = "zip record at %+d, A = %d, decoy %d" % (delta, A, decoy)
        tz.check_index(eng, what, f, device=True, shift=A)
        out, ooff, st = tz.check_read(eng, what, f, device=True, shift=A, out_shift=1)
        assert out[:len(plain)].tobytes() == plain, what
