"""The packed windows of the seek index on the GPU: flate_hip_seek_windows_pack, flate_hip_seek_windows_unpack and
flate_hip_inflate_one_ranges_packed.  Expectations never come from the code under test: the seek index and the raw
windows from tests/seek_ref.py over one_ref.Walk, the keep masks, the sparse windows, the pack index's words and the
read's verdicts from tests/seek_pack_ref.py, the blocks' streams from the oracle encoder, bytes from zlib (plain[b:e]).
The corpus is one_ref.good_streams(oracle), the window-edge streams of one_window_corpus, and a handful of streams
hand-built with deflate_corpus.Writer whose one marked copy sits at each edge of the keep rule."""
import ctypes as C
import random

import numpy as np
import pytest

import deflate_corpus as dc
import one_ref as ref
import one_window_corpus as owc
import seek_pack_ref as sp
import seek_ref as sk
from test_gpu_inflate_one import on_device
from util import flate

pytestmark = pytest.mark.gpu

DEVICE_PTRS = 1
GUARD = 0xA5
GUARD_WORD = 0xA5A5A5A5A5A5A5A5
KINDS = (ref.RAW, ref.ZLIB, ref.GZIP)
SPANS = (1, 4096, 40000, sk.SPAN_NONE)
MODES = (sp.COMPRESS, sp.COMPRESS | sp.SPARSE)
W = sp.WINDOW


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


def edge_streams():
    """Two dynamic blocks -- two units, at span 1 two points, one window -- with ONE copy that reaches in front of the
    second: [(what, raw, plain, the interval of window offsets the rule keeps)].  A: the bytes of the first block,
    dq: literals of the second block in front of the copy."""
    rnd = random.Random(5)
    out = []
    for what, A, dq, ln, dist, want in (
            ("q = P0, distance 32768: the window's first bytes", 40000, 0, 3, 32768, (0, 3)),
            ("q = P0, distance 32767, 258 bytes", 40000, 0, 258, 32767, (1, 259)),
            ("q = P0, distance 1, 258 bytes: an overlapping copy keeps its one source byte", 40000, 0, 258, 1, (W - 1, W)),
            ("q = P0, distance 2, 3 bytes", 40000, 0, 3, 2, (W - 2, W)),
            ("q = P0 + 1, distance 3, 258 bytes: a copy that straddles P0", 40000, 1, 258, 3, (W - 2, W)),
            ("q = P0 + 32767, distance 32768: the last position that counts", 40000, 32767, 3, 32768, (W - 1, W)),
            ("q = P0 + 32768, distance 32768: the first that does not -- an empty block", 40000, 32768, 3, 32768, (0, 0)),
            ("P0 = 100 < 32768, distance 100: the stream's first byte", 100, 0, 3, 100, (W - 100, W - 97))):
        w = dc.Writer()
        lit, dl = dc.full_tree_lens()
        blk = w.dynamic(lit, dl, final=False)
        blk.lits(bytes(rnd.randrange(1, 256) for _ in range(A)))
        blk.end()
        blk = w.dynamic(lit, dl, final=True)
        blk.lits(bytes(rnd.randrange(1, 256) for _ in range(dq)))
        blk.match(ln, dist)
        blk.lits(b"tail")
        blk.end()
        out.append((what, w.data(), bytes(w.out), want))
    return out


class Stream:
    """One stream of the corpus with everything the tests expect of it, computed once per (span, mode)."""

    def __init__(self, what, raw, plain, oracle):
        self.what, self.raw, self.plain, self.oracle = what, raw, plain, oracle
        self.w = ref.Walk(raw)
        self.cps = sp.copies(raw)
        self.memo = {}

    def file(self, kind):
        return ref.wrap(self.raw, self.plain, kind)

    def index(self, kind, span):
        return sk.index_words(self.w, self.plain, len(self.raw), kind, span)

    def expect(self, span, mode):
        """(points, raw windows, the blocks as stored, kept_bytes, off, packed)."""
        if (span, mode) not in self.memo:
            pts = sk.points(self.w.out_off, span)
            blks, kept = sp.blocks(self.plain, self.w.out_off, pts, mode, self.cps)
            off, packed = sp.pack(blks, lambda b: self.oracle.deflate(np.frombuffer(b, np.uint8)))
            self.memo[(span, mode)] = (pts, sk.windows(self.plain, self.w.out_off, pts), blks, kept, off, packed)
        return self.memo[(span, mode)]


@pytest.fixture(scope="module")
def corpus(oracle):
    """{name: [Stream]}: computed once, shared, never changed."""
    return dict(good=[Stream(w, r, p, oracle) for w, r, p in ref.good_streams(oracle)],
                window=[Stream(s[0], s[1], s[2], oracle) for s in owc.good_streams()],
                edge=[Stream(w, r, p, oracle) for w, r, p, _ in edge_streams()])


def buf(data, device, shift, tail=1):
    """data at a shifted address on either side -> (what keeps it alive, its address)."""
    if device:
        return on_device(data, shift)
    keep = np.frombuffer(b"\xee" * shift + bytes(data) + b"\xee" * tail, np.uint8).copy()
    return keep, keep.ctypes.data + shift


def pack(eng, f, kind, words, wins, mode, device=False, shift=0, wshift=0, pshift=0, cap=None, pack_cap=None, no_in=False):
    """One pack call into guarded buffers -> dict(rc, pack_index, packed, pack_words, packed_bytes, kept_bytes)."""
    words = np.ascontiguousarray(words, np.uint64)
    nb = int(words[9]) - 1
    keep_in, in_ptr = buf(f, device, shift)
    keep_w, w_ptr = buf(wins, device, wshift)
    pack_cap = 17 + nb if pack_cap is None else pack_cap
    cap = int(eng._L.flate_hip_seek_windows_pack_bound(nb)) if cap is None else cap
    pidx = np.full(pack_cap + 4, GUARD_WORD, np.uint64)
    pbuf = np.full(pshift + cap + 64, GUARD, np.uint8)
    if device:
        import torch
        d_p = torch.from_numpy(pbuf).cuda()
        p_ptr = d_p.data_ptr() + pshift
    else:
        p_ptr = pbuf.ctypes.data + pshift
    pw, pb, kb = C.c_uint64(99), C.c_uint64(99), C.c_uint64(99)
    rc = eng._L.flate_hip_seek_windows_pack(
        eng._ctx, None if no_in else in_ptr, len(f), kind, words.ctypes.data, len(words), w_ptr if len(wins) else None,
        len(wins), mode, pidx.ctypes.data + 16, pack_cap, C.byref(pw), p_ptr, cap, C.byref(pb), C.byref(kb),
        DEVICE_PTRS if device else 0)
    assert rc != -3, "HIP_FAILURE in the pack: " + eng._L.flate_hip_last_hip_error(eng._ctx).decode()
    if device:
        import torch
        torch.cuda.synchronize()
        pbuf = d_p.cpu().numpy()
    assert (pidx[:2] == GUARD_WORD).all() and (pidx[2 + pack_cap:] == GUARD_WORD).all(), "pack index guard words touched"
    assert (pbuf[:pshift] == GUARD).all() and (pbuf[pshift + cap:] == GUARD).all(), "packed guard bytes touched"
    return dict(rc=rc, pack_index=pidx[2:2 + pack_cap], packed=pbuf[pshift:pshift + cap], pack_words=pw.value,
                packed_bytes=pb.value, kept_bytes=kb.value)


def check_pack(eng, s, kind, span, mode, **kw):
    """The pack equals the reference: the words, the oracle's streams back to back, the kept count."""
    pts, wins, blks, kept, off, packed = s.expect(span, mode)
    index = s.index(kind, span)
    want = sp.pack_words(index, mode, off, kept)
    g = pack(eng, s.file(kind), kind, index, wins, mode, **kw)
    tag = (s.what, kind, span, mode, kw)
    assert (g["rc"], g["pack_words"], g["packed_bytes"], g["kept_bytes"]) == (0, len(want), len(packed), kept), (tag, g["rc"])
    assert [int(x) for x in g["pack_index"]] == want, tag
    assert g["packed"][:len(packed)].tobytes() == packed, tag
    assert (g["packed"][len(packed):] == GUARD).all(), "bytes behind the total touched"
    return index, np.array(want, np.uint64), packed


def unpack(eng, pwords, packed, device=False, pshift=0, wshift=0, cap=None):
    pwords = np.ascontiguousarray(pwords, np.uint64)
    need = int(pwords[3]) * W
    cap = need if cap is None else cap
    keep_p, p_ptr = buf(packed, device, pshift)
    wbuf = np.full(wshift + cap + 64, GUARD, np.uint8)
    if device:
        import torch
        d_w = torch.from_numpy(wbuf).cuda()
        w_ptr = d_w.data_ptr() + wshift
    else:
        w_ptr = wbuf.ctypes.data + wshift
    wb, bad = C.c_uint64(99), C.c_uint32(99)
    rc = eng._L.flate_hip_seek_windows_unpack(eng._ctx, pwords.ctypes.data, len(pwords), p_ptr if len(packed) else None,
                                              len(packed), w_ptr, cap, C.byref(wb), C.byref(bad), DEVICE_PTRS if device else 0)
    assert rc != -3, "HIP_FAILURE in the unpack"
    if device:
        import torch
        torch.cuda.synchronize()
        wbuf = d_w.cpu().numpy()
    assert (wbuf[:wshift] == GUARD).all() and (wbuf[wshift + cap:] == GUARD).all(), "windows guard bytes touched"
    return rc, wb.value, bad.value, wbuf[wshift:wshift + cap]


def read_packed(eng, f, kind, words, pwords, packed, begin, end, cap, device=False, shift=0, pshift=0, out_shift=0,
                query=False):
    """One packed read into a 0xA5-prefilled buffer -> (rc, out_off, range_status, n_decoded, bad_unit, out bytes)."""
    keep, ptr = buf(f, device, shift)
    words, pwords = np.ascontiguousarray(words, np.uint64), np.ascontiguousarray(pwords, np.uint64)
    pk, p_ptr = buf(packed, device, pshift)
    begin, end = np.array(begin, np.uint64), np.array(end, np.uint64)
    nr = len(begin)
    obuf = np.full(out_shift + cap + 64, GUARD, np.uint8)
    if device:
        import torch
        d_out = torch.from_numpy(obuf).cuda()
        out_ptr = d_out.data_ptr() + out_shift
    else:
        out_ptr = obuf.ctypes.data + out_shift
    off, status = np.full(nr + 1, 7, np.uint64), np.full(max(nr, 1), 7, np.int32)
    nd, bad = C.c_uint32(99), C.c_uint32(99)
    rc = eng._L.flate_hip_inflate_one_ranges_packed(
        eng._ctx, ptr, len(f), kind, words.ctypes.data, len(words), pwords.ctypes.data, len(pwords),
        p_ptr if len(packed) else None, len(packed), begin.ctypes.data, end.ctypes.data, nr, None if query else out_ptr,
        0 if query else cap, off.ctypes.data, status.ctypes.data, C.byref(nd), C.byref(bad), DEVICE_PTRS if device else 0)
    assert rc != -3, "HIP_FAILURE in the packed read: " + eng._L.flate_hip_last_hip_error(eng._ctx).decode()
    if device:
        import torch
        torch.cuda.synchronize()
        obuf = d_out.cpu().numpy()
    assert (obuf[:out_shift] == GUARD).all() and (obuf[out_shift + cap:] == GUARD).all(), "guard bytes touched"
    return rc, [int(x) for x in off], [int(x) for x in status[:nr]], nd.value, bad.value, obuf[out_shift:out_shift + cap]


def check_read(eng, s, kind, span, mode, ranges, packed=None, bad_blocks=(), **kw):
    """The packed read equals the model: plain[b:e] back to back, the model's layout, counts and statuses."""
    pts, wins, blks, kept, off, good_packed = s.expect(span, mode)
    index = s.index(kind, span)
    pwords = sp.pack_words(index, mode, off, kept)
    begin, end = [r[0] for r in ranges], [r[1] for r in ranges]
    rc_m, off_m, st_m, nd_m, bad_m, data_m = sp.read(s.plain, s.w.out_off, pts, begin, end, bad_blocks=bad_blocks)
    cap = off_m[-1] + 32
    rc, o, st, nd, bad, body = read_packed(eng, s.file(kind), kind, index, pwords, good_packed if packed is None else packed,
                                           begin, end, cap, **kw)
    tag = (s.what, kind, span, mode, kw)
    assert (rc, o, st, nd, bad) == (rc_m, off_m, st_m, nd_m, bad_m), (tag, rc, rc_m, nd, nd_m, bad, bad_m)
    for r, d in enumerate(data_m):
        if d is not None:  # (the bytes of a range whose status is not 0 are unspecified)
            assert body[o[r]:o[r + 1]].tobytes() == d, (tag, r)
    assert (body[o[-1]:] == GUARD).all(), "bytes behind the total touched"
    return nd


def random_ranges(T, n, seed):
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        b = rnd.randrange(T + 1)
        out.append((b, min(T, b + rnd.choice((0, 1, 7, 300, 5000, 40000)))))
    return out


# ---- the conditions that keep the corpus from going vacuous ----

def test_the_corpus_reaches_every_edge(corpus):
    s = corpus["good"][ref.MANY_UNITS]
    pts, wins, blks, kept, off, packed = s.expect(1, sp.COMPRESS | sp.SPARSE)
    assert len(blks) >= 200 and 0 < kept < len(blks) * W // 20
    for s, n_blocks, n_empty in ((corpus["window"][3], 9, 8), (corpus["window"][22], 71, 70)):  # empty and non-empty mixed
        off = s.expect(1, sp.COMPRESS | sp.SPARSE)[4]
        assert (len(off) - 1, sum(1 for a, b in zip(off, off[1:]) if b == a)) == (n_blocks, n_empty), s.what
    flush = corpus["good"][5]
    assert "Z_FULL_FLUSH" in flush.what and flush.expect(1, 3)[3] == 0 and len(flush.expect(1, 3)[2]) >= 20
    for s, (what, raw, plain, want) in zip(corpus["edge"], edge_streams()):
        pts, wins, blks, kept, off, packed = s.expect(1, sp.COMPRESS | sp.SPARSE)
        assert len(blks) == 1 and kept == want[1] - want[0], what
        mask = sp.keep_masks(s.cps, s.w.out_off, pts)[0]
        assert [i for i, k in enumerate(mask) if k] == list(range(*want)), what
        assert (off[1] == 0) == (want == (0, 0)), what
    assert sum(1 for s in corpus["window"] if s.w.n_units > 1) >= 20


# ---- pack ----

def test_pack_every_stream_at_every_span_in_both_modes(eng, corpus):
    n = 0
    for k, s in enumerate(corpus["good"] + corpus["window"]):
        for j, span in enumerate(SPANS):
            for mode in MODES:
                check_pack(eng, s, KINDS[(k + j) % 3], span, mode)
                n += 1
    assert n > 250


def test_pack_the_edges_of_the_keep_rule(eng, corpus):
    for k, s in enumerate(corpus["edge"]):
        for mode in MODES:
            for device in (False, True):
                check_pack(eng, s, KINDS[k % 3], 1, mode, device=device)
        check_pack(eng, s, ref.RAW, sk.SPAN_NONE, sp.COMPRESS | sp.SPARSE)  # n_points == 1: the head and off = {0}


def test_pack_with_device_pointers_at_odd_alignments(eng, corpus):
    for k in (0, 1, ref.MANY_UNITS, 5, 6, 12):
        s = corpus["good"][k]
        for shift in (0, 1, 3):
            for mode in MODES:
                check_pack(eng, s, KINDS[shift % 3], (4096, 40000, 1)[shift % 3], mode, device=True, shift=shift,
                           wshift=(shift + 1) % 4, pshift=(shift + 2) % 4)
    s = corpus["good"][ref.MANY_UNITS]
    check_pack(eng, s, ref.ZLIB, 4096, sp.COMPRESS | sp.SPARSE, shift=3, wshift=1, pshift=5)


def test_pack_without_the_stream_in_compress_mode(eng, corpus):
    s = corpus["good"][ref.MANY_UNITS]
    for device in (False, True):
        check_pack(eng, s, ref.GZIP, 4096, sp.COMPRESS, device=device, no_in=True)


def test_pack_capacities(eng, corpus):
    s = corpus["good"][ref.MANY_UNITS]
    for mode in MODES:
        pts, wins, blks, kept, off, packed = s.expect(4096, mode)
        index = s.index(ref.GZIP, 4096)
        f = s.file(ref.GZIP)
        for device in (False, True):
            g = pack(eng, f, ref.GZIP, index, wins, mode, device=device, cap=len(packed) - 1, pshift=1)
            assert (g["rc"], g["packed_bytes"], g["pack_words"]) == (-2, len(packed), 17 + len(blks)), (mode, device)
            g = pack(eng, f, ref.GZIP, index, wins, mode, device=device, cap=len(packed), pshift=3)  # the exact total
            assert g["rc"] == 0 and g["packed"].tobytes() == packed, (mode, device)
            g = pack(eng, f, ref.GZIP, index, wins, mode, device=device, pack_cap=16 + len(blks))
            assert (g["rc"], g["pack_words"]) == (-2, 17 + len(blks)), (mode, device)
            assert (g["pack_index"] == GUARD_WORD).all() and (g["packed"] == GUARD).all()  # nothing written


# ---- unpack ----

def test_unpack_gives_the_reference_windows_and_the_unchanged_read_delivers_through_them(eng, corpus):
    from test_gpu_one_seek import read
    for s, span, kind in ((corpus["good"][ref.MANY_UNITS], 4096, ref.GZIP), (corpus["good"][0], 1, ref.RAW),
                          (corpus["good"][5], 1, ref.ZLIB), (corpus["window"][3], 1, ref.GZIP), (corpus["edge"][4], 1, ref.RAW)):
        for mode in MODES:
            pts, wins, blks, kept, off, packed = s.expect(span, mode)
            index = s.index(kind, span)
            pwords = sp.pack_words(index, mode, off, kept)
            for device in (False, True):
                rc, wb, bad, body = unpack(eng, pwords, packed, device=device, pshift=1 if device else 0, wshift=3 if device else 0)
                assert (rc, wb, bad) == (0, len(wins), 0xffffffff), (s.what, mode, device)
                assert body.tobytes() == (b"".join(blks) if mode & sp.SPARSE else wins), (s.what, mode, device)
            ranges = sk.edge_ranges(s.w.out_off, pts)[:60]
            begin, end = [r[0] for r in ranges], [r[1] for r in ranges]
            rc_m, off_m, st_m, nd_m, bad_m, data_m = sk.read(s.plain, s.w.out_off, pts, begin, end)
            rc, o, st, nd, bad, out = read(eng, s.file(kind), kind, index, body.tobytes(), begin, end, off_m[-1] + 32)
            assert (rc, o, st, nd, bad) == (rc_m, off_m, st_m, nd_m, bad_m), (s.what, mode)
            assert out[:o[-1]].tobytes() == b"".join(data_m), (s.what, mode)
    s = corpus["good"][ref.MANY_UNITS]
    pts, wins, blks, kept, off, packed = s.expect(4096, 3)
    pwords = sp.pack_words(s.index(ref.GZIP, 4096), 3, off, kept)
    rc, wb, bad, body = unpack(eng, pwords, packed, cap=len(wins) - 1)
    assert (rc, wb) == (-2, len(wins)) and (body == GUARD).all()


# ---- the packed read ----

def test_read_packed_equals_the_model(eng, corpus):
    n = 0
    for k, s in enumerate(corpus["good"] + corpus["window"][::3] + corpus["edge"]):
        for j, span in enumerate(SPANS):
            pts = sk.points(s.w.out_off, span)
            ranges = sk.edge_ranges(s.w.out_off, pts)
            ranges = ranges[:len(ranges) // 2][:120] + random_ranges(s.w.out_off[-1], 20, k + j)
            mode = MODES[(k + j) % 2]
            n += check_read(eng, s, KINDS[(k + j) % 3], span, mode, ranges, device=bool((k + j) & 1))
    s = corpus["good"][ref.MANY_UNITS]
    for span in (1, 4096, 40000):
        pts = sk.points(s.w.out_off, span)
        for mode in MODES:
            for device in (False, True):
                check_read(eng, s, ref.GZIP, span, mode, sk.edge_ranges(s.w.out_off, pts) + random_ranges(300000, 50, span),
                           device=device, shift=1 if device else 0, pshift=3 if device else 0, out_shift=1)
    assert n > 1500  # (units decoded over all reads)


def test_read_packed_decodes_only_the_selected_blocks(eng, corpus):
    s = corpus["good"][ref.MANY_UNITS]
    pts, wins, blks, kept, off, packed = s.expect(4096, 3)
    k = sk.longest_segment_last(s.w.out_off, pts)
    one = [(s.w.out_off[k + 1] - 1, s.w.out_off[k + 1])]
    p = sk.pstart(pts, k)
    b = pts.index(p) - 1
    # every other block's stream destroyed: the read never looks at them
    junk = bytearray(b"\xff" * len(packed))
    junk[off[b]:off[b + 1]] = packed[off[b]:off[b + 1]]
    for device in (False, True):
        nd = check_read(eng, s, ref.GZIP, 4096, 3, one, packed=bytes(junk), device=device)
        assert nd == k + 1 - p
    # the size query and a short capacity: the raw call's verdict 4
    index, pwords = s.index(ref.GZIP, 4096), sp.pack_words(s.index(ref.GZIP, 4096), 3, off, kept)
    rc, o, st, nd, bad, body = read_packed(eng, s.file(ref.GZIP), ref.GZIP, index, pwords, packed, [0], [1000], 999)
    assert (rc, o, st) == (-2, [0, 1000], [0]) and (body == GUARD).all()
    rc, o, st, nd, bad, body = read_packed(eng, s.file(ref.GZIP), ref.GZIP, index, pwords, packed, [5], [9], 0, query=True)
    assert (rc, o) == (-2, [0, 4])


# ---- failures ----

def test_a_bad_block_fails_its_own_ranges_and_no_others(eng, corpus):
    s = corpus["good"][ref.MANY_UNITS]
    span, mode = 4096, sp.COMPRESS | sp.SPARSE
    pts, wins, blks, kept, off, packed = s.expect(span, mode)
    full = [b for b in range(len(blks)) if off[b + 1] > off[b]]
    b = full[len(full) // 2]
    ranges = sk.edge_ranges(s.w.out_off, pts)
    flipped = bytearray(packed)
    flipped[off[b]] ^= 0x06  # the first header's block type: a reserved type or a stored block of garbage lengths
    for device in (False, True):
        check_read(eng, s, ref.GZIP, span, mode, ranges, packed=bytes(flipped), bad_blocks=(b,), device=device)
    # cut short: the stream of block b loses its second half, the offsets say so, the blocks behind it are intact
    half = (off[b + 1] - off[b]) // 2
    cut = packed[:off[b] + half] + packed[off[b + 1]:]
    off2 = off[:b + 1] + [x - (off[b + 1] - off[b] - half) for x in off[b + 1:]]
    index = s.index(ref.GZIP, span)
    pwords = sp.pack_words(index, mode, off2, kept)
    begin, end = [r[0] for r in ranges], [r[1] for r in ranges]
    want = sp.read(s.plain, s.w.out_off, pts, begin, end, bad_blocks=(b,))
    rc, o, st, nd, bad, body = read_packed(eng, s.file(ref.GZIP), ref.GZIP, index, pwords, cut, begin, end, want[1][-1] + 32)
    assert (rc, o, st, nd, bad) == want[:5] and rc == -4 and bad == pts[b + 1]
    for r, d in enumerate(want[5]):
        if d is not None:
            assert body[o[r]:o[r + 1]].tobytes() == d, r
    assert sum(1 for x in st if x) > 0 and sum(1 for x in st if not x) > len(st) // 2
    # and unpack names the block
    rc, wb, bad, body = unpack(eng, pwords, cut)
    assert (rc, bad) == (-4, b)
    good_w = b"".join(blks)
    assert body[:b * W].tobytes() == good_w[:b * W] and body[(b + 1) * W:].tobytes() == good_w[(b + 1) * W:]


def test_a_pack_index_from_another_index_is_refused(eng, corpus):
    s = corpus["good"][ref.MANY_UNITS]
    pts, wins, blks, kept, off, packed = s.expect(4096, 3)
    index = s.index(ref.GZIP, 4096)
    other = corpus["good"][4]
    o_exp = other.expect(4096, 3)
    o_words = sp.pack_words(other.index(ref.GZIP, 4096), 3, o_exp[4], o_exp[3])
    rc, o, st, nd, bad, body = read_packed(eng, s.file(ref.GZIP), ref.GZIP, index, o_words, o_exp[5], [0], [10], 64)
    assert rc == -1 and (body == GUARD).all() and o == [7, 7]  # nothing written
    spanned = sp.pack_words(s.index(ref.GZIP, 40000), 3, off, kept)  # the same stream at another span
    rc, o, st, nd, bad, body = read_packed(eng, s.file(ref.GZIP), ref.GZIP, index, spanned, packed, [0], [10], 64)
    assert rc == -1 and (body == GUARD).all()


def test_another_stream_of_the_same_length_is_corrupt(eng, corpus):
    s = corpus["good"][ref.MANY_UNITS]
    span = 4096
    pts, wins, blks, kept, off, packed = s.expect(span, 3)
    for kind in (ref.ZLIB, ref.GZIP):
        index = s.index(kind, span)
        f = bytearray(s.file(kind))
        f[-1] ^= 1  # the trailer's last byte: the checksum (zlib) or ISIZE (gzip)
        for device in (False, True):
            g = pack(eng, bytes(f), kind, index, wins, 3, device=device)
            assert g["rc"] == -4, (kind, device)
            pwords = sp.pack_words(index, 3, off, kept)
            rc, o, st, nd, bad, body = read_packed(eng, bytes(f), kind, index, pwords, packed, [0, 5], [10, 9], 64, device=device)
            assert (rc, o, st) == (-4, [0, 0, 0], [-4, -4]) and (body == GUARD).all()
    # a raw stream has no trailer: other bits of the same length are found by the walk, which leaves the segment's blocks
    # or ends them anywhere but at the segment's end bit
    index = s.index(ref.RAW, span)
    i = len(pts) // 2
    ub, oo = s.w.unit_bit, s.w.out_off
    seg = (ub[pts[i]], ub[pts[i + 1]], oo[pts[i + 1]] - oo[pts[i]], False)
    assert seg[2] <= W and sp.segment_fits(s.raw, *seg)
    other = bytearray(s.raw)
    at = seg[0] // 8 + 40
    other[at:at + 64] = b"\xff" * 64
    assert at + 64 < seg[1] // 8 and not sp.segment_fits(bytes(other), *seg)  # (the reference's verdict, not the library's)
    for device in (False, True):
        g = pack(eng, bytes(other), ref.RAW, index, wins, 3, device=device)
        assert g["rc"] == -4, device
    g = pack(eng, bytes(other), ref.RAW, index, wins, sp.COMPRESS)  # without SPARSE the stream is not read at all
    assert g["rc"] == 0 and g["packed"][:g["packed_bytes"]].tobytes() == s.expect(span, sp.COMPRESS)[5]


def test_refusals_come_before_any_hip_call_with_nothing_written(eng, corpus):
    s = corpus["good"][ref.MANY_UNITS]
    pts, wins, blks, kept, off, packed = s.expect(4096, 3)
    index = s.index(ref.GZIP, 4096)
    f = s.file(ref.GZIP)
    for mode in (0, 2, 4, 7):
        g = pack(eng, f, ref.GZIP, index, wins, mode)
        assert g["rc"] == -1 and (g["pack_index"] == GUARD_WORD).all() and (g["packed"] == GUARD).all(), mode
        assert (g["pack_words"], g["packed_bytes"], g["kept_bytes"]) == (99, 99, 99), mode
    g = pack(eng, f, ref.GZIP, index, wins, 3, no_in=True)  # SPARSE walks the stream
    assert g["rc"] == -1 and g["pack_words"] == 99
    bent = list(index)
    bent[sk.HEAD_WORDS + 2] = bent[sk.HEAD_WORDS + 1]  # unit_bit repeats: seek_index_ok refuses it
    g = pack(eng, f, ref.GZIP, bent, wins, 3)
    assert g["rc"] == -1 and g["pack_words"] == 99
