"""The tile geometry of flate_hip_inflate_one_index's discovery: one workgroup tests every bit offset of a 4 KiB tile
(plus 16 bytes of halo) on the grid of the buffer's ADDRESS, inside the raw stream's range [raw_off, raw_end) of a
container.  Here a dynamic block header is PLACED: a stored block of n zero bytes in front moves it to any byte around a
tile boundary, a fixed block in front of it to any bit phase, the device tensor's shift to any alignment; and bytes that
would complete a cut header stand where a container's trailer is.  Every expectation is the Python walker's and the
Python rule's (tests/one_ref.py: Walk, rule, candidates) on the same bytes, the content zlib's; a candidate the
discovery misses stops the chain at a header the tail probe accepts, which is FLATE_HIP_E_INTERNAL."""
import struct
import zlib

import pytest

import deflate_corpus as dc
import gzip_ref
import one_ref as ref
from test_gpu_inflate_one import check_index, index
from test_gpu_inflate_one_read import check_good, read
from util import flate

gpu = pytest.mark.gpu  # (the one test without it checks the placed streams themselves, on the CPU)

TILE = 4096  # kTileBytes
OFFSETS = tuple(range(-17, 2))  # the header's byte against the tile boundary: the last 11 bytes of a tile read the halo
LIT, DIST = dc.small_lens()


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


def make_tail(phase):
    """(bytes, what they inflate to, the byte that holds the first dynamic header's first bit -- at bit `phase`)."""
    w = dc.Writer()
    dc.prefix_block(w, phase)
    hbit = w.pos
    assert hbit % 8 == phase
    blk = w.dynamic(LIT, DIST, final=False)
    dc.dyn_body(blk)
    blk.end()
    blk = w.dynamic(LIT, DIST, final=True)
    blk.lits(dc.TEXT[:9])
    blk.match(4, 2)
    blk.end()
    assert w.marks["cl_syms"] - w.marks["block"] == 74  # 3 + 14 + 19 * 3 bits: at phase 7 the head test reads 81
    return w.data(), bytes(w.out), hbit // 8


TAILS = [make_tail(phase) for phase in range(8)]
# the rule's hits in a tail, counted from the second zero byte in front of it (no hit starts in zero bytes: the type
# bits of a dynamic header are 10)
TAIL_HITS = [len([b for b in ref.candidates(bytes(2) + t[0]) if b]) for t in TAILS]


def placed(n, phase):
    """The stream with n zero bytes stored in front of tail[phase] -> (raw, plain, the header's byte in raw, candidates)."""
    tail, out, hbyte = TAILS[phase]
    raw = b"\x00" + struct.pack("<HH", n, n ^ 0xffff) + bytes(n) + tail
    head = raw[:5 + 600]  # (a header is shorter than 600 bytes: the rule's verdict at the first 40 bits lies in here)
    n_cand = 1 + sum(1 for b in range(1, 40) if ref.rule(head, b)) + TAIL_HITS[phase]
    return raw, bytes(n) + out, 5 + n + hbyte, n_cand


def test_the_placed_streams_are_what_they_claim():
    """On the CPU: zlib reads them, the header is at its bit, and the candidate count by parts equals the count over the
    whole stream."""
    for phase in range(8):
        raw, plain, p, n_cand = placed(700 + 37 * phase, phase)
        assert zlib.decompress(raw, -15) == plain
        w = ref.Walk(raw)
        assert (w.status, w.n_units) == (0, 3) and w.unit_bit[1] == 8 * p + phase
        assert ref.rule(raw, 8 * p + phase) and n_cand == len(ref.candidates(raw))


@gpu
@pytest.mark.parametrize("A", (0, 1, 8, 15))
def test_a_header_at_every_byte_and_bit_around_a_tile_boundary(eng, A):
    """v = A + raw_off + (the header's byte) runs over 4096 k - 17 .. 4096 k + 1."""
    for kind in (ref.RAW, ref.GZIP):
        for k in (1, 2):
            for delta in OFFSETS:
                for phase in range(8):
                    n = TILE * k + delta - A - ref.header_len(kind) - 5 - TAILS[phase][2]
                    raw, plain, p, n_cand = placed(n, phase)
                    assert A + ref.header_len(kind) + p == TILE * k + delta
                    w = ref.Walk(raw)
                    assert (w.status, w.n_units, w.unit_bit[1]) == (0, 3, 8 * p + phase)
                    what = "header at tile %d %+d, bit %d, A = %d" % (k, delta, phase, A)
                    assert check_index(eng, raw, plain, w, what, kind, device=True, shift=A) == n_cand, what
                    if phase == (delta + 17) % 8:
                        check_good(eng, raw, plain, w, what, kind, device=True, shift=A, out_shift=1)


def small_stream(blocks):
    w = dc.Writer()
    for i in range(blocks):
        blk = w.dynamic(LIT, DIST, final=i == blocks - 1)
        dc.dyn_body(blk)
        blk.end()
    return w.data(), bytes(w.out)


@gpu
@pytest.mark.parametrize("A", (1, 15))
def test_first_chunk_at_an_unaligned_address(eng, A):
    """The stream starts with a dynamic block at a pointer that is not 16-aligned: the byte-wise branch of tile_load."""
    raw, plain = small_stream(2)
    w = ref.Walk(raw)
    assert zlib.decompress(raw, -15) == plain and w.n_units == 2
    for kind in (ref.RAW, ref.GZIP):
        nc = check_index(eng, raw, plain, w, "first chunk", kind, device=True, shift=A)
        assert nc == len(ref.candidates(raw)), (A, kind, nc)
        check_good(eng, raw, plain, w, "first chunk", kind, device=True, shift=A)


@gpu
def test_last_chunk_ends_with_the_final_dynamic_block(eng):
    raw, plain = small_stream(3)
    w = ref.Walk(raw)
    assert zlib.decompress(raw, -15) == plain and w.n_units == 3 and w.end_bit > 8 * (len(raw) - 1)
    want = len(ref.candidates(raw))
    for kind in (ref.RAW, ref.ZLIB):
        in_len = len(ref.wrap(raw, plain, kind))
        for rest in (0, 1, 15):
            A = (rest - in_len) % 16
            assert check_index(eng, raw, plain, w, "last chunk", kind, device=True, shift=A) == want, (kind, rest)
            check_good(eng, raw, plain, w, "last chunk", kind, device=True, shift=A)


@gpu
def test_nothing_behind_raw_end_is_read(eng):
    """A stream cut inside its last dynamic header, and where the container's trailer stands the bytes that would
    complete the header: for the rule they are absent."""
    w = dc.Writer()
    blk = w.dynamic(LIT, DIST, final=False)
    dc.dyn_body(blk)
    blk.end()
    hbit = w.pos
    blk = w.dynamic(LIT, DIST, final=True)
    h_end = (w.marks["body"] + 7) // 8  # the header lies in raw[hbit // 8 : h_end]
    blk.lits(dc.TEXT)
    blk.end()
    raw = w.data()
    assert ref.rule(raw, hbit) and len(raw) >= h_end + 8
    for kind, n_tr, head in ((ref.GZIP, 8, gzip_ref.header()), (ref.ZLIB, 4, b"\x78\x9c")):
        bites = 0
        cuts = sorted(set(range(hbit // 8 + 1, hbit // 8 + 13)) | set(range(h_end - n_tr, h_end)))
        for cut in cuts:
            assert hbit // 8 < cut < h_end and not ref.rule(raw[:cut], hbit)
            bites += ref.rule(raw[:cut + n_tr], hbit)  # a rule that read the trailer's bytes would take the header
            f = head + raw[:cut] + raw[cut:cut + n_tr]
            wc = ref.Walk(raw[:cut])
            assert (wc.status, wc.n_units, wc.unit_bit) == (ref.UNEXPECTED_EOF, 1, [0, hbit])
            rc, nu, ob, nc, st, eo, ubit, ooff = index(eng, f, kind, wc.n_units, device=True, shift=cut % 3)
            assert nc == len(ref.candidates(raw[:cut])), (kind, cut, nc)
            assert (rc, st, nu, ob, eo) == (wc.status, wc.status, wc.n_units, 0, -1), (kind, cut, rc, st, nu)
            assert list(ubit[:nu + 1]) == wc.unit_bit and list(ooff[:nu + 1]) == wc.out_off, (kind, cut)
            rc, got, ol, st, eo, nu, nc, _ = read(eng, f, kind, wc.out_len + 64, device=True, shift=cut % 3)
            assert (rc, st, ol, nu) == (wc.status, wc.status, wc.out_len, 1), (kind, cut, rc, st, ol)
            assert got == bytes(w.out[:wc.out_len]), (kind, cut)
        assert bites == n_tr, (kind, bites)
